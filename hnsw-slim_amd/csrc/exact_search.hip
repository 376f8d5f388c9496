// exact_search.hip -- exact k-NN over the rows a resident index already holds, in the format it holds them (fp32, or the u8 /
// fp16 narrow copy), under the index's delete marks and, optionally, a filter set with one filter per query.
//
// The answer of query i is the min(k, #candidates) lexicographically smallest (dist, label) pairs over its candidates: the
// internal ids that are not marked deleted and, when a filter set is named, whose bit is set in the query's filter row -- the
// exclusion rule of FilterArgs (engine.hpp).  Without filter and delete marks that is hnswlib::BruteforceSearch::searchKnn
// (bruteforce.h:106-135) over the index's (row, label) pairs, bit for bit.  With a filter it is NOT the reference's filtered
// overload: that code takes `lastdist` from a queue that may hold fewer than k entries (bruteforce.h:118-131) and then drops
// nearer allowed rows depending on the scan order; here the result does not depend on the order of the rows.
//
// Geometry: brute_force.hip's -- a workgroup of 4 waves, a tile of 8 queries in LDS, a chunk of rows per workgroup, a sorted k-list
// per (wave, query), sorted runs, then its merge kernel.  What differs:
//  * rows: a template parameter selects fp32 (DevIndex::vec) or the narrow copy in its lane-major layout (narrow_rows.hip), read four
//    lanes per row as beam_search.hip's wave_dists reads it and widened by narrow_load.hpp; element 16 i + 4 sub + j still reaches
//    accumulator j of lane sub in step order i, so a distance has the bits it has from the fp32 row;
//  * admission: a wave works in units of one bitmap word (32 rows).  It reads the tile's eight filter words of the unit once,
//    clears the deleted rows and the rows beyond n, and skips the unit before any row is loaded when the union over the tile is
//    empty (wave uniform).  A row is offered to query t only if t's word has its bit: one more term of the ballot next to d <= thr;
//  * query order: tile slot s serves query order[s] (outputs stay at the query's position), so that a caller -- the host entry
//    does -- can put queries of one filter into one tile; a selective filter then costs about the rows it allows, not n.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bf_common.hpp"
#include "bf_engine.hpp"
#include "exact_engine.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

static constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct ExactScan {
  const void *rows;          // fp32 rows or the narrow copy
  const uint64_t *labels;
  const uint8_t *deleted;    // null: the index has no delete marks
  const float *queries;
  const uint32_t *order;     // nullable
  BfEntry *partial;
  FilterArgs f;              // f.rows == null: no filter set
  uint32_t n, dim, nq, k, rows_per_block;
};

struct ExactLds {
  float *q;            // kQT x dim
  BfEntry *lists;      // kWaves x kQT x k
  uint32_t *sizes;     // kWaves x kQT
  uint32_t *slot_q;    // kQT: the query a tile slot serves, kNoSlot beyond nq
  uint32_t *slot_f;    // kQT: its filter row (0 without a filter set), kNoSlot = nothing is admitted
};

// Stages the tile: which query and filter row each slot has, the queries, empty lists.
__device__ __forceinline__ ExactLds exact_stage(const ExactScan &a, unsigned char *smem, int tid) {
  ExactLds s;
  s.q = reinterpret_cast<float *>(smem);
  s.lists = reinterpret_cast<BfEntry *>(smem + (((size_t)kQT * a.dim * 4 + 15) & ~(size_t)15));
  s.sizes = reinterpret_cast<uint32_t *>(s.lists + (size_t)kWaves * kQT * a.k);
  s.slot_q = s.sizes + kWaves * kQT;
  s.slot_f = s.slot_q + kQT;
  const uint32_t q0 = blockIdx.y * kQT;
  if (tid < kQT) {
    uint32_t qi = kNoSlot, fi = kNoSlot;
    if (q0 + tid < a.nq) {
      qi = a.order ? a.order[q0 + tid] : q0 + tid;
      if (qi >= a.nq) qi = kNoSlot;
    }
    if (qi != kNoSlot) {
      if (!a.f.rows) fi = 0;
      else {
        const uint32_t fo = a.f.of_query[qi];
        if (fo < a.f.nf) fi = fo;
        else if (blockIdx.x == 0) atomicAdd(a.f.bad, 1u);   // once per query: its first row chunk
      }
    }
    s.slot_q[tid] = qi;
    s.slot_f[tid] = fi;
  }
  if (tid < kWaves * kQT) s.sizes[tid] = 0;
  __syncthreads();
  for (uint32_t i = tid; i < kQT * a.dim; i += 64 * kWaves) {
    const uint32_t t = i / a.dim, qi = s.slot_q[t];
    s.q[i] = qi != kNoSlot ? a.queries[(size_t)qi * a.dim + (i - t * a.dim)] : 0.f;
  }
  __syncthreads();
  return s;
}

// Admission word of unit u (rows 32 u .. 32 u + 31, 32 u < n) in lane t < kQT for tile slot t: the slot's filter word, less the
// deleted rows and the rows beyond n.  Zero in the other lanes and for a slot that admits nothing.
__device__ __forceinline__ uint32_t exact_admit(const ExactScan &a, const ExactLds &s, uint32_t u, int lane) {
  const uint32_t base = u * 32, left = a.n - base;
  uint32_t alive = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
  if (a.deleted) {
    const uint32_t idx = base + ((uint32_t)lane & 31u);
    const bool del = lane < 32 && idx < a.n && a.deleted[idx] != 0;
    alive &= ~(uint32_t)hs_ballot(del);
  }
  uint32_t w = 0;
  if (lane < kQT) {
    const uint32_t fi = s.slot_f[lane];
    if (fi != kNoSlot) w = a.f.rows ? a.f.rows[(size_t)fi * a.f.stride + u] : 0xFFFFFFFFu;
  }
  return w & alive;
}

// Sorted runs of this (chunk, wave), padded with +inf, for the merge kernel: at the position of the query a slot serves.
__device__ __forceinline__ void exact_write_runs(const ExactScan &a, const ExactLds &s, int wave, int lane) {
  const BfEntry *mine = s.lists + (size_t)wave * kQT * a.k;
  const uint32_t *msz = s.sizes + wave * kQT;
  const uint32_t run = blockIdx.x * kWaves + wave, nruns = gridDim.x * kWaves;
  for (int t = 0; t < kQT; t++) {
    const uint32_t qi = s.slot_q[t];
    if (qi == kNoSlot) continue;
    BfEntry *dst = a.partial + ((size_t)qi * nruns + run) * a.k;
    for (uint32_t i = lane; i < a.k; i += 64) dst[i] = i < msz[t] ? mine[(size_t)t * a.k + i] : BfEntry{INFINITY, 0xFFFFFFFFu, ~0ull};
  }
}

// dim % 16 == 0: 4 lanes per row, 16 rows per pass, two passes per unit.
template <int METRIC, typename ROW>
__device__ __forceinline__ void exact_scan_body(const ExactScan &a, unsigned char *smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 3, grp = lane >> 2;
  const ExactLds s = exact_stage(a, smem, tid);
  const float *q = s.q;
  const uint32_t dim = a.dim, k = a.k;
  BfEntry *mine = s.lists + (size_t)wave * kQT * k;
  uint32_t *msz = s.sizes + wave * kQT;
  const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const uint32_t steps = dim >> 4;
  for (uint32_t u = (r0 >> 5) + wave; u * 32 < r1; u += kWaves) {
    const uint32_t w = exact_admit(a, s, u, lane);
    uint32_t aw[kQT], un = 0;
#pragma unroll
    for (int t = 0; t < kQT; t++) {
      aw[t] = __builtin_amdgcn_readlane(w, t);
      un |= aw[t];
    }
    if (!un) continue;   // nobody in the tile may see a row of this unit: nothing is loaded
#pragma unroll 1
    for (uint32_t h = 0; h < 32; h += 16) {
      if (!((un >> h) & 0xFFFFu)) continue;
      const uint32_t rb = u * 32 + h, row = rb + grp;
      const bool act = (un >> (h + grp)) & 1u;
      const size_t at = (size_t)(act ? row : r0) * dim;   // idle groups re-read the chunk's first row and discard
      float acc[kQT][4];
#pragma unroll
      for (int t = 0; t < kQT; t++) acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f;
      if constexpr (RowKind<ROW>::narrow) {
        // the lane's two chunks of the row (narrow_rows.hip): pairs (16 i + 4 sub, + 1) and (16 i + 4 sub + 2, + 3), i = 0 .. steps - 1
        const ROW *ca = static_cast<const ROW *>(a.rows) + at + (uint32_t)sub * (dim >> 2), *cb = ca + 2 * steps;
        const bool aligned4 = sizeof(ROW) == 2 || !(steps & 1u);   // both chunks start on a dword
        for (uint32_t s0 = 0; s0 < steps; s0 += 8) {
          const uint32_t nb = min(8u, steps - s0);
          const uint32_t nw = aligned4 ? (nb & ~3u) : 0u;   // pairs of this round that come in wide loads
          NarrowRound<ROW> ra, rc;
          ra.load(ca + 2 * s0, nb, nw);
          rc.load(cb + 2 * s0, nb, nw);
#pragma unroll
          for (uint32_t i = 0; i < 8; i++)
            if (i < nb) {
              const hs_f2 xa = ra.pair(i, nw), xb = rc.pair(i, nw);
              const float4 xv = make_float4(xa.x, xa.y, xb.x, xb.y);
#pragma unroll
              for (int t = 0; t < kQT; t++) {
                const float4 qv = *reinterpret_cast<const float4 *>(q + (size_t)t * dim + (s0 + i) * 16 + sub * 4);
                step4<METRIC>(acc[t], qv, xv);
              }
            }
        }
      } else {
        const float4 *x = reinterpret_cast<const float4 *>(static_cast<const float *>(a.rows) + at) + sub;
        for (uint32_t st = 0; st < steps; st++) {
          const float4 xv = x[st * 4];
#pragma unroll
          for (int t = 0; t < kQT; t++) {
            const float4 qv = *reinterpret_cast<const float4 *>(q + (size_t)t * dim + st * 16 + sub * 4);
            step4<METRIC>(acc[t], qv, xv);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < kQT; t++) {
        bool owner;
        const float d = lane4_reduce<METRIC>(acc[t], sub, owner);
        if (!((aw[t] >> h) & 0xFFFFu)) continue;   // (wave uniform)
        const uint32_t sz = msz[t];
        const float thr = sz < k ? INFINITY : mine[(size_t)t * k + k - 1].d;
        const bool adm = (aw[t] >> (h + grp)) & 1u;
        bf_offer<2>(hs_ballot(adm && owner && d <= thr), d, rb, a.labels, mine + (size_t)t * k, msz + t, k, lane);   // bruteforce.h:120 `dist <= lastdist`
      }
    }
  }
  wave_sync();
  exact_write_runs(a, s, wave, lane);
}

// Register budgets: left alone the compiler takes 110 VGPRs for the fp32 body (4 waves per SIMD) and ~140 for the narrow ones (3), to
// keep more row loads in flight than this scan can use -- it is bound by the vector ALU, as bf_scan_kernel is (83 VGPRs, 5 waves for
// L2).  Asking for bf_scan_kernel's occupancy gives the fp32 body 82 VGPRs and no scratch; the narrow bodies, which hold a round of
// packed row words next to the accumulators, spill at 4 waves and are left at 3.
#define HS_WAVES_PER_SIMD(n) __attribute__((amdgpu_waves_per_eu(n)))
template <int METRIC>
__global__ void __launch_bounds__(64 * kWaves) HS_WAVES_PER_SIMD(5) exact_scan_kernel(const ExactScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  exact_scan_body<METRIC, float>(a, smem);
}
template <int METRIC>
__global__ void __launch_bounds__(64 * kWaves) exact_scan_kernel_u8(const ExactScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  exact_scan_body<METRIC, uint8_t>(a, smem);
}
template <int METRIC>
__global__ void __launch_bounds__(64 * kWaves) exact_scan_kernel_f16(const ExactScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  exact_scan_body<METRIC, _Float16>(a, smem);
}

// dim % 16 != 0 (fp32 rows only): the reference's SIMD4 / residual / scalar recipes (dist_recipe.hpp l2_general / ip_general), one
// lane per row, 64 rows = two units per wave and pass, as brute_force.hip's bf_scan_general_kernel.
template <int METRIC>
__global__ void __launch_bounds__(64 * kWaves) exact_scan_general_kernel(const ExactScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ExactLds s = exact_stage(a, smem, tid);
  const uint32_t dim = a.dim, k = a.k;
  BfEntry *mine = s.lists + (size_t)wave * kQT * k;
  uint32_t *msz = s.sizes + wave * kQT;
  const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  for (uint32_t rb = r0 + wave * 64; rb < r1; rb += 64 * kWaves) {
    const uint32_t w0 = exact_admit(a, s, rb >> 5, lane);
    const uint32_t w1 = rb + 32 < r1 ? exact_admit(a, s, (rb >> 5) + 1, lane) : 0u;
    const unsigned long long un = hs_ballot(lane < kQT && (w0 | w1) != 0);
    if (!un) continue;   // no slot admits a row of these two units
    const uint32_t row = rb + lane;
    const float *x = static_cast<const float *>(a.rows) + (size_t)(row < r1 ? row : r0) * dim;
#pragma unroll 1
    for (int t = 0; t < kQT; t++) {
      const uint32_t lo = __builtin_amdgcn_readlane(w0, t), hi = __builtin_amdgcn_readlane(w1, t);   // (the builtin returns int: no sign extension)
      const unsigned long long at = ((unsigned long long)hi << 32) | lo;
      if (!at) continue;   // (wave uniform)
      const float d = METRIC == METRIC_L2 ? l2_general(s.q + (size_t)t * dim, x, dim) : ip_general(s.q + (size_t)t * dim, x, dim);
      const uint32_t sz = msz[t];
      const float thr = sz < k ? INFINITY : mine[(size_t)t * k + k - 1].d;
      const bool adm = (at >> lane) & 1ull;
      bf_offer<0>(hs_ballot(adm && d <= thr), d, rb, a.labels, mine + (size_t)t * k, msz + t, k, lane);
    }
  }
  wave_sync();
  exact_write_runs(a, s, wave, lane);
}

size_t exact_lds_bytes(uint32_t dim, uint32_t k) {
  return (((size_t)kQT * dim * 4 + 15) & ~(size_t)15) + (size_t)kWaves * kQT * k * sizeof(BfEntry) + (kWaves * kQT + 2 * kQT) * 4;
}

hipError_t launch_exact_search(const DevIndex &ix, const void *rows, int fmt, const ExactArgs &a, const FilterArgs *f, hipStream_t stream) {
  const size_t lds = exact_lds_bytes(ix.dim, a.k);
  if (lds > 160 * 1024) return hipErrorInvalidValue;   // the query tile no longer fits the CU's LDS
  const bool general = (ix.dim & 15u) != 0;
  if (general && fmt != ROWS_F32) return hipErrorInvalidValue;   // narrow rows exist for dim % 16 == 0 only
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2;
  void (*kern)(const ExactScan) =
      general ? (l2 ? exact_scan_general_kernel<METRIC_L2> : exact_scan_general_kernel<METRIC_IP>)
      : fmt == ROWS_U8 ? (l2 ? exact_scan_kernel_u8<METRIC_L2> : exact_scan_kernel_u8<METRIC_IP>)
      : fmt == ROWS_F16 ? (l2 ? exact_scan_kernel_f16<METRIC_L2> : exact_scan_kernel_f16<METRIC_IP>)
                        : (l2 ? exact_scan_kernel<METRIC_L2> : exact_scan_kernel<METRIC_IP>);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  ExactScan sa{};
  sa.rows = rows; sa.labels = ix.labels; sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.queries = a.queries; sa.order = a.order; sa.partial = static_cast<BfEntry *>(a.partial);
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = ix.dim; sa.nq = a.nq; sa.k = a.k; sa.rows_per_block = a.rows_per_block;
  const dim3 grid(a.grid_x, (a.nq + kQT - 1) / kQT);
  hipLaunchKernelGGL(kern, grid, dim3(64 * kWaves), lds, stream, sa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_bf_merge(a.partial, a.nq, a.k, a.grid_x * kWaves, a.out_labels, a.out_dists, a.out_counts, stream);
}

}  // namespace hs
