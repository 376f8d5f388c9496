// exact_range_screen.hip -- exact range search over a resident index's rows by screen, re-rank and fallback.  The
// answer is exact_range.hip's, bit for bit: offsets, labels, fp32 distance bits, order.
//
// Why that holds: a query's answer is the set of candidates with r <= radius, r the recipe's distance, sorted by (dist, label).  For
// an admitted row the screen computes a (L2: |q|^2 + |x|^2 - 2 q.x, IP: 1 - q.x; the dot product by v_mfma_f32_32x32x2f32) and
// e = exact_screen_margin with |a - r| <= e, so r >= lo = a - e.  r <= radius implies lo <= radius: keeping the rows with
// lo <= radius keeps a superset of the answer, and the recipe over the superset with the test r <= radius is the answer.  The
// threshold is the caller's and fixed before the first row is read: no running bound, no list in LDS, no merge.
//
// xrs_screen_kernel  exact_screen.hip's geometry: a workgroup of 4 waves, a tile of 64 queries in LDS as fp32 in operand layout, a
//                    chunk of rows; wave (b, p) owns the 32 queries of half b and the 32-row units of parity p, one 32 x 32
//                    accumulator block per unit, rows straight from global memory in stored order with the next load in flight
//                    under the MFMAs.  LDS holds the tile and 16 bytes per query, so the tile stays whole up to dim 624 (464 for
//                    the k-NN screen at k = 10); a longer one goes through in slices of 128 positions, four blocks per wave.
//                    Epilogue per accumulator element: a, e, lo, hi, admission as exact_search.hip's, lo <= radius[q].  Survivors
//                    are a ballot; the lanes of a half-wave share a query, so one of them takes popcount positions from the
//                    query's cursor in device memory with one atomic add and each survivor stores its row id at its own position of
//                    the query's list while that is below kXrsList.  The cursor counts on beyond it.
// xrs_rerank_kernel  one wave per query.  A query with a raised flag (an admitted pair whose interval is not finite) or a cursor above
//                    kXrsList goes to the fallback order, flagged queries first.  For the others: r of each listed row four lanes per
//                    row by xs_recipe_dist (the scan's step4 / lane4_reduce), r <= radius as an fp32 comparison, the kept (row, r)
//                    compacted in place, the hit count to counts[query][0] and zeros to the query's other chunks.
// fallback           exact_range.hip's count and fill kernels over the fallback order, enqueued behind the re-rank; they read the
//                    number of flagged queries on the device and a tile beyond it returns at once.
// xrs_copy_kernel    the kept (dist, label) of an unflagged query to out_offsets[q], under the fill's total <= cap rule.
// Overflow: a query falls back iff its cursor's final value exceeds kXrsList.  The value is the number of its survivors, a function
// of the inputs; which survivors reached the list first does not enter.  Up to kXrsList every survivor is in the list.
// The object is built without the packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bf_common.hpp"
#include "exact_range_screen_engine.hpp"
#include "exact_screen_margin.hpp"
#include "exact_screen_rows.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

// clears what a call accumulates (no memset node: the sequence may be captured)
__global__ void __launch_bounds__(256) xrs_init_kernel(uint32_t *state, uint32_t *qflag, uint32_t *fb_order, uint32_t *cursor, uint32_t nq) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nq) { qflag[i] = 0; fb_order[i] = kXsNoSlot; cursor[i] = 0; }
  if (i < kXsStateWords) state[i] = 0;   // (the first workgroup has 256 threads)
}

// ---- screen ------------------------------------------------------------------------------------------------------------------
struct XrsScan {
  const void *rows;
  const uint8_t *deleted;
  const float *queries, *radius, *xn, *qn;
  const uint32_t *order;
  uint32_t *qflag, *cursor, *lists;
  FilterArgs f;
  uint32_t n, dim, nq, rows_per_block, slice;
};

// NU: 32-row units a wave carries at a time, one accumulator block each: 1 for a tile staged whole, else the units that share one
// staging of a slice (exact_screen.hip xs_screen_body has the walk; the epilogue is this file's).
template <int METRIC, typename ROW, int NU>
__device__ __forceinline__ void xrs_screen_body(const XrsScan &a, unsigned char *smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = wave & 1, p = wave >> 1, j = lane & 31, h = lane >> 5;
  const uint32_t dim = a.dim, slice = a.slice;
  float *qL = reinterpret_cast<float *>(smem);                       // (slice / 8) x 2 x 64 x 4
  float *qn2 = qL + (size_t)kXsTile * slice;                         // 64
  float *rad = qn2 + kXsTile;                                        // 64: NaN for a slot without a query
  uint32_t *slot_q = reinterpret_cast<uint32_t *>(rad + kXsTile);    // 64
  uint32_t *slot_f = slot_q + kXsTile;                               // 64
  const uint32_t q0 = blockIdx.x * kXsTile;
  if (tid < (int)kXsTile) {
    uint32_t qi = kXsNoSlot, fi = kXsNoSlot;
    if (q0 + tid < a.nq) {
      qi = a.order ? a.order[q0 + tid] : q0 + tid;
      if (qi >= a.nq) qi = kXsNoSlot;
    }
    if (qi != kXsNoSlot) {
      if (!a.f.rows) fi = 0;
      else {
        const uint32_t fo = a.f.of_query[qi];
        if (fo < a.f.nf) fi = fo;
        else if (blockIdx.y == 0) atomicAdd(a.f.bad, 1u);   // once per query: its first row chunk
      }
    }
    slot_q[tid] = qi;
    slot_f[tid] = fi;
    qn2[tid] = qi != kXsNoSlot ? a.qn[qi] : 0.f;
    rad[tid] = qi != kXsNoSlot ? a.radius[qi] : __uint_as_float(0x7FC00000u);
  }
  __syncthreads();
  const bool whole = slice >= dim;
  if (whole) {
    xs_stage<ROW>(qL, slot_q, a.queries, dim, 0, dim, tid);
    __syncthreads();
  }

  const uint32_t r0 = blockIdx.y * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const float4 *qA = reinterpret_cast<const float4 *>(qL) + h * kXsTile + 32 * b + j;   // + 128 per chunk of 8 positions
  // (the trip count is the workgroup's: every wave meets the barriers of the sliced form)
  for (uint32_t ug = r0 >> 5; ug * 32 < r1; ug += 2 * NU) {
    // admission word of local slot `lane` (lanes 0 .. 31) per unit, as exact_search.hip's exact_admit; 0 for a unit beyond the chunk
    uint32_t w[NU];
    bool act[NU];
    xs_f16v acc[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) {
      const uint32_t u = ug + p + 2 * i, base = u * 32;
      w[i] = 0;
      if (base < r1) {
        const uint32_t left = a.n - base;
        uint32_t alive = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
        if (a.deleted) {
          const uint32_t idx = base + j;
          const bool del = lane < 32 && idx < a.n && a.deleted[idx] != 0;
          alive &= ~(uint32_t)hs_ballot(del);
        }
        if (lane < 32) {
          const uint32_t fi = slot_f[32 * b + lane];
          if (fi != kXsNoSlot) w[i] = a.f.rows ? a.f.rows[(size_t)fi * a.f.stride + u] : 0xFFFFFFFFu;
        }
        w[i] &= alive;
      }
      act[i] = hs_ballot(w[i] != 0) != 0;   // no query of this half may see a row of the unit: nothing of it is loaded
#pragma unroll
      for (int v = 0; v < 16; v++) acc[i][v] = 0.f;
    }
    for (uint32_t p0 = 0; p0 < dim; p0 += slice) {
      const uint32_t len = min(slice, dim - p0), nc = len >> 3;
      if (!whole) {
        __syncthreads();   // every wave is done with the slice before
        xs_stage<ROW>(qL, slot_q, a.queries, dim, p0, len, tid);
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < NU; i++) {
        if (!act[i]) continue;
        const uint32_t row = (ug + p + 2 * i) * 32 + j;
        const ROW *x = static_cast<const ROW *>(a.rows) + (size_t)(row < a.n ? row : r0) * dim + p0;   // rows beyond n re-read the chunk's first
        XsChunk<ROW> cur;
        cur.load(x, h, 0);
        for (uint32_t cc = 0; cc < nc; cc++) {
          XsChunk<ROW> nxt = cur;
          if (cc + 1 < nc) nxt.load(x, h, cc + 1);
          const float4 xb = cur.wide();
          const float4 qa = qA[(size_t)cc * 2 * kXsTile];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.x, xb.x, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.y, xb.y, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.z, xb.z, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.w, xb.w, acc[i], 0, 0, 0);
          cur = nxt;
        }
      }
    }
    // element v of lane (j, h): query slot 8 (v / 4) + 4 h + v % 4 of the half against row j of the unit -- the 32 lanes of a
    // half-wave hold 32 rows against one query
#pragma unroll
    for (int i = 0; i < NU; i++) {
      if (!act[i]) continue;
      const uint32_t row = (ug + p + 2 * i) * 32 + j;
      const float xnl = row < a.n ? a.xn[row] : 0.f;
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const uint32_t tl = 8u * (v >> 2) + 4u * h + (v & 3), t = 32 * b + tl;
        const uint32_t awv = (uint32_t)__shfl((int)w[i], (int)tl);
        const bool adm = (awv >> j) & 1u;   // (an admitted pair has a query: slot_f says so)
        const float qq = qn2[t], rq = rad[t];
        const float dot = acc[i][v];
        const float av = METRIC == METRIC_L2 ? (qq + xnl) - 2.f * dot : 1.f - dot;
        const float e = exact_screen_margin(METRIC == METRIC_IP, dim, qq, xnl);
        const float lo = av - e, hi = av + e;
        const bool fin = (lo - lo == 0.f) && (hi - hi == 0.f);
        if (adm && !fin && rq == rq) a.qflag[slot_q[t]] = 1;   // (several lanes may write the same 1; a NaN radius admits nothing anyway)
        const bool surv = adm && fin && lo <= rq;
        const unsigned long long m = hs_ballot(surv);
        if (!m) continue;
        const uint32_t mine = (uint32_t)(m >> (32 * h));                   // the survivors of this lane's query
        const int lead = mine ? __ffs((int)mine) - 1 : 0;
        uint32_t at = 0;
        if (surv && (int)j == lead) at = atomicAdd(a.cursor + slot_q[t], (uint32_t)__popc(mine));
        at = (uint32_t)__shfl((int)at, (int)(32 * h) + lead);
        if (surv) {
          const uint32_t pos = at + (uint32_t)__popc(mine & ((1u << j) - 1u));
          if (pos < kXrsList) a.lists[(size_t)slot_q[t] * (2 * kXrsList) + pos] = row;
        }
      }
    }
  }
}

#define HS_XRS_SCREEN(NAME, ROW)                                                \
  template <int METRIC, int NU>                                                 \
  __global__ void __launch_bounds__(256) NAME(const XrsScan a) {                \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];        \
    xrs_screen_body<METRIC, ROW, NU>(a, smem);                                  \
  }
HS_XRS_SCREEN(xrs_screen_kernel, float)
HS_XRS_SCREEN(xrs_screen_kernel_u8, uint8_t)
HS_XRS_SCREEN(xrs_screen_kernel_i8, int8_t)
HS_XRS_SCREEN(xrs_screen_kernel_f16, _Float16)
HS_XRS_SCREEN(xrs_screen_kernel_bf16, hs_bf16)
HS_XRS_SCREEN(xrs_screen_kernel_f8, hs_f8)
#undef HS_XRS_SCREEN

// ---- re-rank and count -------------------------------------------------------------------------------------------------------
struct XrsRerank {
  const void *rows;
  const float *queries, *radius;
  const uint32_t *cursor;
  uint32_t *qflag, *state, *fb_order, *lists, *counts;
  uint32_t dim, nq, chunks;
};

template <int METRIC, typename ROW>
__device__ __forceinline__ void xrs_rerank_body(const XrsRerank &a, float *q) {
  const uint32_t qi = blockIdx.x, dim = a.dim;
  const int lane = threadIdx.x, sub = lane & 3, grp = lane >> 2;
  const uint32_t cnt = a.cursor[qi];
  if (a.qflag[qi] != 0 || cnt > kXrsList) {   // (wave uniform) the passes behind this kernel serve the query; its counts are theirs
    if (lane == 0) {
      a.qflag[qi] = 1;
      a.fb_order[atomicAdd(a.state + 0, 1u)] = qi;
      atomicAdd(a.state + 1, 1u);
    }
    return;
  }
  for (uint32_t c = 1 + lane; c < a.chunks; c += 64) a.counts[(size_t)qi * a.chunks + c] = 0;
  for (uint32_t i = lane; i < dim; i += 64) q[i] = a.queries[(size_t)qi * dim + i];
  wave_sync();
  const float rq = a.radius[qi];
  uint32_t *L = a.lists + (size_t)qi * (2 * kXrsList);
  float *D = reinterpret_cast<float *>(L + kXrsList);
  uint32_t kc = 0;
  // 16 listed rows per pass.  The kept ones go back into the list at kc .. < e0 + 16: below everything a later pass reads, and
  // behind this pass's own reads, which the ballot has waited for.
  for (uint32_t e0 = 0; e0 < cnt; e0 += 16) {
    const uint32_t idx = e0 + grp;
    const bool act = idx < cnt;
    const uint32_t row = act ? L[idx] : 0u;   // idle groups take row 0 and discard (cnt > 0: the index holds a row)
    bool owner;
    const float d = xs_recipe_dist<METRIC, ROW>(q, a.rows, (size_t)row * dim, dim, sub, owner);
    const bool keep = act && owner && d <= rq;
    const unsigned long long mask = hs_ballot(keep);
    if (keep) {
      const uint32_t pos = kc + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      L[pos] = row;
      D[pos] = d;
    }
    kc += (uint32_t)__popcll(mask);
  }
  if (lane == 0) {
    a.counts[(size_t)qi * a.chunks] = kc;
    atomicAdd(reinterpret_cast<unsigned long long *>(a.state + 2), (unsigned long long)cnt);
  }
}

#define HS_XRS_RERANK(NAME, ROW)                                                \
  template <int METRIC>                                                         \
  __global__ void __launch_bounds__(64) NAME(const XrsRerank a) {               \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];        \
    xrs_rerank_body<METRIC, ROW>(a, reinterpret_cast<float *>(smem));           \
  }
HS_XRS_RERANK(xrs_rerank_kernel, float)
HS_XRS_RERANK(xrs_rerank_kernel_u8, uint8_t)
HS_XRS_RERANK(xrs_rerank_kernel_i8, int8_t)
HS_XRS_RERANK(xrs_rerank_kernel_f16, _Float16)
HS_XRS_RERANK(xrs_rerank_kernel_bf16, hs_bf16)
HS_XRS_RERANK(xrs_rerank_kernel_f8, hs_f8)
#undef HS_XRS_RERANK

// ---- copy --------------------------------------------------------------------------------------------------------------------
// One workgroup per query: the kept entries of an unflagged query to its segment.  counts[q][0] of them lie in its list, and
// [offsets[q], offsets[q] + counts[q][0]) is its whole segment, inside [0, total) and so inside the outputs when total <= cap.
__global__ void __launch_bounds__(256) xrs_copy_kernel(const uint32_t *qflag, const uint32_t *lists, const uint32_t *counts, uint32_t chunks,
                                                       const uint64_t *offsets, uint32_t nq, uint64_t cap, const uint64_t *labels,
                                                       uint64_t *out_labels, float *out_dists, uint32_t *over) {
  const uint32_t qi = blockIdx.x, tid = threadIdx.x;
  if (offsets[nq] > cap) {
    if (tid == 0 && qi == 0) atomicOr(over, 1u);
    return;
  }
  if (qflag[qi] != 0) return;
  const uint32_t kc = min(counts[(size_t)qi * chunks], kXrsList);
  const uint64_t b = offsets[qi];
  const uint32_t *L = lists + (size_t)qi * (2 * kXrsList);
  const float *D = reinterpret_cast<const float *>(L + kXrsList);
  for (uint32_t i = tid; i < kc; i += 256) {
    const uint32_t row = L[i];
    out_dists[b + i] = D[i];
    out_labels[b + i] = labels ? labels[row] : (uint64_t)row;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kXrsSlice = 128;   // positions per slice of a tile that does not fit whole
static constexpr int kXrsSliceUnits = 4;     // units a wave carries per slice (NU)
static constexpr size_t kXrsLdsBudget = 160 * 1024;
static size_t xrs_lds_for(uint32_t slice) { return (size_t)kXsTile * slice * 4 + 4 * kXsTile * 4; }
uint32_t xrs_whole_dim() { return (uint32_t)((kXrsLdsBudget - 4 * kXsTile * 4) / (kXsTile * 4)) & ~15u; }
uint32_t xrs_slice(uint32_t dim) { return dim <= xrs_whole_dim() ? dim : kXrsSlice; }
bool xrs_supported(uint32_t dim) { return dim != 0 && (dim & 15u) == 0 && dim <= 4096; }
void xrs_plan(uint32_t n, uint32_t nq, uint32_t *grid_y, uint32_t *rows_per_block) {
  // enough workgroups to fill the chip for few queries (exact_screen.hip xs_plan); a chunk is a multiple of 64 rows: whole unit pairs
  const uint32_t tiles = (nq + kXsTile - 1) / kXsTile;
  uint32_t gy = tiles ? (1024 + tiles - 1) / tiles : 1;
  gy = gy < 1 ? 1 : (gy > 64 ? 64 : gy);
  uint32_t rpb = (uint32_t)((((uint64_t)n + gy - 1) / gy + 63) / 64 * 64);
  if (rpb < 512) rpb = 512;
  gy = (uint32_t)(((uint64_t)n + rpb - 1) / rpb);
  if (gy == 0) gy = 1;
  *grid_y = gy;
  *rows_per_block = rpb;
}
const char *xrs_kernel_name(int fmt) {
  return fmt == ROWS_U8 ? "hs::xrs_screen_kernel_u8" : fmt == ROWS_I8 ? "hs::xrs_screen_kernel_i8" : fmt == ROWS_BF16 ? "hs::xrs_screen_kernel_bf16" : fmt == ROWS_F8 ? "hs::xrs_screen_kernel_f8" : fmt == ROWS_F16 ? "hs::xrs_screen_kernel_f16" : "hs::xrs_screen_kernel";
}

// the fallback's arguments: the flagged queries, found on the device
static RangeArgs xrs_fallback(const RangeScreenArgs &a) {
  RangeArgs fb = a.r;
  fb.order = a.fb_order;
  fb.live = a.state;
  return fb;
}

hipError_t launch_exact_range_screen_count(const DevIndex &ix, const void *rows, int fmt, const RangeScreenArgs &a, const FilterArgs *f, hipStream_t stream) {
  const uint32_t dim = ix.dim, nq = a.r.nq;
  if (!xrs_supported(dim) || nq == 0 || a.grid_y == 0 || (a.rows_per_block & 63u)) return hipErrorInvalidValue;
  if ((uint64_t)a.grid_y * a.rows_per_block < ix.n) return hipErrorInvalidValue;   // the chunks cover the rows
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  if (!a.r.queries || !a.r.radius || !a.r.counts || !a.xnorm2 || !a.qnorm2 || !a.state || !a.qflag || !a.fb_order || !a.cursor || !a.lists)
    return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2;
  hipError_t e;
  hipLaunchKernelGGL(xrs_init_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, a.state, a.qflag, a.fb_order, a.cursor, nq);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_exact_screen_norms(ix, rows, fmt, a.xnorm2, stream)) != hipSuccess) return e;
  if ((e = launch_exact_screen_qnorms(a.r.queries, nq, dim, a.qnorm2, stream)) != hipSuccess) return e;

  const uint32_t slice = xrs_slice(dim);
  void (*screen)(const XrsScan);
#define HS_XRS_PICK(NU)                                                                                                        \
  screen = fmt == ROWS_U8     ? (l2 ? xrs_screen_kernel_u8<METRIC_L2, NU> : xrs_screen_kernel_u8<METRIC_IP, NU>)                 \
           : fmt == ROWS_I8   ? (l2 ? xrs_screen_kernel_i8<METRIC_L2, NU> : xrs_screen_kernel_i8<METRIC_IP, NU>)                 \
           : fmt == ROWS_BF16 ? (l2 ? xrs_screen_kernel_bf16<METRIC_L2, NU> : xrs_screen_kernel_bf16<METRIC_IP, NU>)             \
           : fmt == ROWS_F8   ? (l2 ? xrs_screen_kernel_f8<METRIC_L2, NU> : xrs_screen_kernel_f8<METRIC_IP, NU>)                 \
           : fmt == ROWS_F16  ? (l2 ? xrs_screen_kernel_f16<METRIC_L2, NU> : xrs_screen_kernel_f16<METRIC_IP, NU>)               \
                              : (l2 ? xrs_screen_kernel<METRIC_L2, NU> : xrs_screen_kernel<METRIC_IP, NU>)
  if (slice >= dim) HS_XRS_PICK(1);
  else HS_XRS_PICK(kXrsSliceUnits);
#undef HS_XRS_PICK
  const size_t lds = xrs_lds_for(slice);
  if (lds > 48 * 1024) {   // beyond the default limit of dynamic LDS: asked for by name
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(screen), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  XrsScan sa{};
  sa.rows = rows; sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.queries = a.r.queries; sa.radius = a.r.radius; sa.xn = a.xnorm2; sa.qn = a.qnorm2; sa.order = a.r.order;
  sa.qflag = a.qflag; sa.cursor = a.cursor; sa.lists = a.lists;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = dim; sa.nq = nq; sa.rows_per_block = a.rows_per_block; sa.slice = slice;
  hipLaunchKernelGGL(screen, dim3((nq + kXsTile - 1) / kXsTile, a.grid_y), dim3(256), lds, stream, sa);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  void (*rerank)(const XrsRerank) = fmt == ROWS_U8     ? (l2 ? xrs_rerank_kernel_u8<METRIC_L2> : xrs_rerank_kernel_u8<METRIC_IP>)
                                    : fmt == ROWS_I8   ? (l2 ? xrs_rerank_kernel_i8<METRIC_L2> : xrs_rerank_kernel_i8<METRIC_IP>)
                                    : fmt == ROWS_BF16 ? (l2 ? xrs_rerank_kernel_bf16<METRIC_L2> : xrs_rerank_kernel_bf16<METRIC_IP>)
                                    : fmt == ROWS_F8   ? (l2 ? xrs_rerank_kernel_f8<METRIC_L2> : xrs_rerank_kernel_f8<METRIC_IP>)
                                    : fmt == ROWS_F16  ? (l2 ? xrs_rerank_kernel_f16<METRIC_L2> : xrs_rerank_kernel_f16<METRIC_IP>)
                                                       : (l2 ? xrs_rerank_kernel<METRIC_L2> : xrs_rerank_kernel<METRIC_IP>);
  XrsRerank ra{};
  ra.rows = rows; ra.queries = a.r.queries; ra.radius = a.r.radius; ra.cursor = a.cursor;
  ra.qflag = a.qflag; ra.state = a.state; ra.fb_order = a.fb_order; ra.lists = a.lists; ra.counts = a.r.counts;
  ra.dim = dim; ra.nq = nq; ra.chunks = a.r.chunks;
  hipLaunchKernelGGL(rerank, dim3(nq), dim3(64), (size_t)dim * 4, stream, ra);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the flagged queries' rows of the count matrix, then the exclusive scan of all of it: always enqueued
  return launch_exact_range_count(ix, rows, fmt, xrs_fallback(a), f, stream);
}

hipError_t launch_exact_range_screen_fill(const DevIndex &ix, const void *rows, int fmt, const RangeScreenArgs &a, const FilterArgs *f, hipStream_t stream) {
  const uint32_t nq = a.r.nq;
  if (nq == 0) return hipErrorInvalidValue;
  if (!a.r.over || (a.r.cap && (!a.r.out_labels || !a.r.out_dists))) return hipErrorInvalidDevicePointer;
  hipLaunchKernelGGL(xrs_copy_kernel, dim3(nq), dim3(256), 0, stream, a.qflag, a.lists, a.r.counts, a.r.chunks, a.r.out_offsets, nq, a.r.cap, ix.labels,
                     a.r.out_labels, a.r.out_dists, a.r.over);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_exact_range_fill(ix, rows, fmt, xrs_fallback(a), f, stream);
}

}  // namespace hs
