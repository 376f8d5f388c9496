// exact_range.hip -- exact range search over the rows of a resident index: every candidate of exact_search.hip whose distance is
// <= the query's radius, in CSR form (offsets, labels, distances), ascending by (dist, label) inside a query's segment.
//
// The k-NN scans keep a bounded list per query; a range result has no bound, so nothing is kept on chip:
//  * count pass: grid = (tiles of 8 queries) x (row chunks); a workgroup walks its chunk in rounds of 128 rows, one 32-row unit per
//    wave (256 rows and two units per wave for dim % 16 != 0, one lane per row), with no barrier inside the walk.  A row is a hit of
//    slot t if its bit is in t's admission word (filter row, less deleted rows and rows beyond n, as exact_search.hip) and
//    dist <= radius[t].  The hits of a pass are a ballot; its popcount goes to the slot's counter in LDS.  At the end the eight
//    counters go to counts[query][chunk].  LDS holds the query tile and 32 bytes per slot: the waves of a CU are the limit, not LDS;
//  * offsets: xr_offsets_kernel, one workgroup, the exclusive scan of the count matrix in query-major order (a contiguous slice per
//    thread, a scan of the 256 slice sums in LDS): bases[query][chunk], out_offsets[query], out_offsets[nq] = the total;
//  * fill pass: the same kernel text with FILL = true, the same walk and the same distances.  The hit lanes of a pass take
//    bases[query][chunk] + (one LDS atomic add per wave on the slot's counter) + (the lane's ballot prefix) and store (dist, label)
//    there.  The order inside a (query, chunk) piece is whatever the waves' atomics gave;
//  * segment sort: xr_sort_kernel, one workgroup per query, sorts [out_offsets[q], out_offsets[q + 1]) by (dist, label) with a
//    bitonic network written for any length: every merge stage opens with a mirrored step (i against size - 1 - i of its block) and
//    every comparison ascends, so the +inf entries that would pad the segment to a power of two would never move and a partner
//    beyond the segment is skipped.  Up to kRangeSortLds entries the segment is sorted in LDS; a longer one runs the same network
//    on device memory, in place, one barrier per step -- the slow path.  A segment of 0 or 1 entries returns at once.
// Capacity: fill and sort read the total from out_offsets[nq]; above cap they store nothing but the `over` word.  Below it a store
// is still guarded by the end of its (query, chunk) piece, so no store can leave the outputs.
// Determinism: (dist, label) is a total order on a query's hits (labels are unique), so the sorted segment does not depend on the
// order the fill appended in.
// Distances: exact_search.hip's passes as exact_wide.hip duplicates them -- four lanes per row, element 16 i + 4 sub + j reaches
// accumulator j of lane sub in step i, lane4_reduce; l2_general / ip_general for dim % 16 != 0 -- so a hit has the bits
// hs_index_exact_search gives.  No matrix or dot-product instruction is involved.  The object is built without the packed fp32
// instructions (Makefile).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bf_common.hpp"
#include "exact_range_engine.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

static constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
static constexpr int kRangeThreads = 64 * kWaves;

struct RangeScan {
  const void *rows;          // fp32 rows or the narrow copy
  const uint64_t *labels;
  const uint8_t *deleted;    // null: the index has no delete marks
  const float *queries, *radius;
  const uint32_t *order;     // nullable
  const uint32_t *live;      // nullable: the first *live slots of `order` name queries; a tile beyond them returns at once
  uint32_t *counts;          // nq x gridDim.y: written by the count pass, read by the fill pass
  const uint64_t *bases;     // nq x gridDim.y (fill)
  const uint64_t *total;     // out_offsets + nq (fill)
  uint64_t cap;
  uint64_t *out_labels;
  float *out_dists;
  uint32_t *over;
  FilterArgs f;              // f.rows == null: no filter set
  uint32_t n, dim, nq, rows_per_chunk;
};

struct RangeLds {
  float *q;            // kQT x dim
  uint64_t *base;      // kQT: where the slot's (query, chunk) piece starts (fill)
  uint64_t *end;       // kQT: and where it ends
  float *rad;          // kQT: NaN for a slot without a query
  uint32_t *slot_q;    // kQT: the query a tile slot serves, kNoSlot beyond nq
  uint32_t *slot_f;    // kQT: its filter row (0 without a filter set), kNoSlot = nothing is admitted
  uint32_t *cnt;       // kQT: hits so far
};

// Add on a word of LDS as the DS instruction itself (wave_util.hpp lds_cas has the reason).
__device__ __forceinline__ uint32_t xr_lds_add(uint32_t *p, uint32_t v) {
  const uint32_t addr = (uint32_t)(uintptr_t)p;
  uint32_t old;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(v) : "memory");
  return old;
}

// Stages the tile: which query, filter row and radius each slot has, the queries, the counters; for the fill the pieces' bounds.
template <bool FILL>
__device__ __forceinline__ RangeLds xr_stage(const RangeScan &a, unsigned char *smem, int tid) {
  RangeLds s;
  s.q = reinterpret_cast<float *>(smem);
  s.base = reinterpret_cast<uint64_t *>(smem + (((size_t)kQT * a.dim * 4 + 15) & ~(size_t)15));
  s.end = s.base + kQT;
  s.rad = reinterpret_cast<float *>(s.end + kQT);
  s.slot_q = reinterpret_cast<uint32_t *>(s.rad + kQT);
  s.slot_f = s.slot_q + kQT;
  s.cnt = s.slot_f + kQT;
  const uint32_t q0 = blockIdx.x * kQT;
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
        else if (!FILL && blockIdx.y == 0) atomicAdd(a.f.bad, 1u);   // once per query: its first row chunk, the count pass
      }
    }
    s.slot_q[tid] = qi;
    s.slot_f[tid] = fi;
    s.rad[tid] = qi != kNoSlot ? a.radius[qi] : __uint_as_float(0x7FC00000u);
    s.cnt[tid] = 0;
    uint64_t b = 0, e = 0;
    if (FILL && qi != kNoSlot) {
      const size_t at = (size_t)qi * gridDim.y + blockIdx.y;
      b = a.bases[at];
      e = b + a.counts[at];
    }
    s.base[tid] = b;
    s.end[tid] = e;
  }
  __syncthreads();
  for (uint32_t i = tid; i < kQT * a.dim; i += kRangeThreads) {
    const uint32_t t = i / a.dim, qi = s.slot_q[t];
    s.q[i] = qi != kNoSlot ? a.queries[(size_t)qi * a.dim + (i - t * a.dim)] : 0.f;
  }
  __syncthreads();
  return s;
}

// Admission word of unit u (rows 32 u .. 32 u + 31, 32 u < n) in lane t < kQT for tile slot t (exact_search.hip exact_admit).
__device__ __forceinline__ uint32_t xr_admit(const RangeScan &a, const RangeLds &s, uint32_t u, int lane) {
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

// The lanes of mask m (not empty; the whole wave is here) are hits of slot t: counted, or stored at the piece's cursor.
template <bool FILL>
__device__ __forceinline__ void xr_hits(const RangeScan &a, const RangeLds &s, uint32_t t, unsigned long long m, float d, uint32_t row, int lane) {
  uint32_t at = 0;
  if (lane == 0) at = xr_lds_add(s.cnt + t, (uint32_t)__popcll(m));
  if (!FILL) return;
  at = uni(at);
  if ((m >> lane) & 1ull) {
    const uint64_t pos = s.base[t] + at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < s.end[t]) {   // (always, while the rows are those the count pass saw: no store leaves the piece)
      a.out_dists[pos] = d;
      a.out_labels[pos] = a.labels ? a.labels[row] : (uint64_t)row;
    }
  }
}

// One 32-row unit of a wave, dim % 16 == 0: 4 lanes per row, 16 rows per pass, two passes (exact_search.hip exact_scan_body).
template <int METRIC, typename ROW, bool FILL>
__device__ __forceinline__ void xr_unit(const RangeScan &a, const RangeLds &s, uint32_t u, uint32_t r0, int lane) {
  const int sub = lane & 3, grp = lane >> 2;
  const float *q = s.q;
  const uint32_t dim = a.dim, steps = dim >> 4;
  const uint32_t w = xr_admit(a, s, u, lane);
  uint32_t aw[kQT], un = 0;
#pragma unroll
  for (int t = 0; t < kQT; t++) {
    aw[t] = __builtin_amdgcn_readlane(w, t);
    un |= aw[t];
  }
  if (!un) return;   // nobody in the tile may see a row of this unit: nothing is loaded
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
      const bool adm = (aw[t] >> (h + grp)) & 1u;
      const unsigned long long m = hs_ballot(adm && owner && d <= s.rad[t]);
      if (m) xr_hits<FILL>(a, s, t, m, d, row, lane);
    }
  }
}

// The count pass leaves the slots' counters in counts[query][chunk].
__device__ __forceinline__ void xr_finish_count(const RangeScan &a, const RangeLds &s, int tid) {
  __syncthreads();
  if (tid < kQT && s.slot_q[tid] != kNoSlot) a.counts[(size_t)s.slot_q[tid] * gridDim.y + blockIdx.y] = s.cnt[tid];
}

// The fill pass stands still when the results do not fit (the whole workgroup takes the same way: a.total is read by all).
__device__ __forceinline__ bool xr_fill_refused(const RangeScan &a, int tid) {
  if (*a.total <= a.cap) return false;
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) atomicOr(a.over, 1u);
  return true;
}

// A subset found on the device (exact_range_screen.hip's fallback): the slots at and beyond *a.live name no query, so the tile has
// nothing to count or fill (the whole workgroup takes the same way).  Without a.live every tile runs.
__device__ __forceinline__ bool xr_tile_idle(const RangeScan &a) { return a.live && blockIdx.x * kQT >= *a.live; }

template <int METRIC, typename ROW, bool FILL>
__device__ __forceinline__ void xr_scan_body(const RangeScan &a, unsigned char *smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (FILL && xr_fill_refused(a, tid)) return;
  if (xr_tile_idle(a)) return;
  const RangeLds s = xr_stage<FILL>(a, smem, tid);
  const uint32_t r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint32_t u = (r0 >> 5) + wave; u * 32 < r1; u += kWaves) xr_unit<METRIC, ROW, FILL>(a, s, u, r0, lane);
  if (!FILL) xr_finish_count(a, s, tid);
}

#define HS_RANGE_KERNEL(NAME, ROW)                                                                \
  template <int METRIC, bool FILL>                                                                \
  __global__ void __launch_bounds__(kRangeThreads) NAME(const RangeScan a) {                      \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                          \
    xr_scan_body<METRIC, ROW, FILL>(a, smem);                                                     \
  }
HS_RANGE_KERNEL(exact_range_kernel, float)
HS_RANGE_KERNEL(exact_range_kernel_u8, uint8_t)
HS_RANGE_KERNEL(exact_range_kernel_i8, int8_t)
HS_RANGE_KERNEL(exact_range_kernel_f16, _Float16)
HS_RANGE_KERNEL(exact_range_kernel_bf16, hs_bf16)
HS_RANGE_KERNEL(exact_range_kernel_f8, hs_f8)
#undef HS_RANGE_KERNEL

// dim % 16 != 0 (fp32 rows only): dist_recipe.hpp's l2_general / ip_general, one lane per row, 64 rows = two units per wave and
// round, as exact_search.hip's exact_scan_general_kernel.
template <int METRIC, bool FILL>
__global__ void __launch_bounds__(kRangeThreads) exact_range_general_kernel(const RangeScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (FILL && xr_fill_refused(a, tid)) return;
  if (xr_tile_idle(a)) return;
  const RangeLds s = xr_stage<FILL>(a, smem, tid);
  const uint32_t dim = a.dim;
  const uint32_t r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint32_t wb = r0 + wave * 64; wb < r1; wb += 64 * kWaves) {
    const uint32_t w0 = xr_admit(a, s, wb >> 5, lane);
    const uint32_t w1 = wb + 32 < r1 ? xr_admit(a, s, (wb >> 5) + 1, lane) : 0u;
    if (!hs_ballot(lane < kQT && (w0 | w1) != 0)) continue;   // no slot admits a row of these two units
    const uint32_t row = wb + lane;
    const float *x = static_cast<const float *>(a.rows) + (size_t)(row < r1 ? row : r0) * dim;
#pragma unroll 1
    for (uint32_t t = 0; t < kQT; t++) {
      const uint32_t lo = __builtin_amdgcn_readlane(w0, t), hi = __builtin_amdgcn_readlane(w1, t);
      const unsigned long long at = ((unsigned long long)hi << 32) | lo;
      if (!at) continue;   // (wave uniform)
      const float d = METRIC == METRIC_L2 ? l2_general(s.q + (size_t)t * dim, x, dim) : ip_general(s.q + (size_t)t * dim, x, dim);
      const bool adm = (at >> lane) & 1ull;
      const unsigned long long m = hs_ballot(adm && d <= s.rad[t]);
      if (m) xr_hits<FILL>(a, s, t, m, d, row, lane);
    }
  }
  if (!FILL) xr_finish_count(a, s, tid);
}

// One workgroup: the exclusive scan of counts[0 .. nq * chunks) (query-major) into bases, the value at every query's first chunk
// into offsets, the sum into offsets[nq].  A thread sums a contiguous slice, the 256 sums are scanned in LDS, the slice is walked again.
__global__ void __launch_bounds__(kRangeThreads) xr_offsets_kernel(const uint32_t *counts, uint32_t nq, uint32_t chunks, uint64_t *bases,
                                                                    uint64_t *offsets) {
  __shared__ uint64_t part[kRangeThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t total = (uint64_t)nq * chunks, per = (total + kRangeThreads - 1) / kRangeThreads;
  const uint64_t b = tid * per < total ? tid * per : total, e = b + per < total ? b + per : total;
  uint64_t sum = 0;
  for (uint64_t i = b; i < e; i++) sum += counts[i];
  part[tid] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < kRangeThreads; off <<= 1) {
    const uint64_t v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint64_t run = part[tid] - sum;
  for (uint64_t i = b; i < e; i++) {
    bases[i] = run;
    if (i % chunks == 0) offsets[i / chunks] = run;
    run += counts[i];
  }
  if (tid == kRangeThreads - 1) offsets[nq] = part[tid];
}

// Bitonic network for any length n over the pairs (d[i], l[i]), ascending by (dist, label), by the workgroup: the +inf entries that
// would pad n to a power of two stay where they are under ascending comparisons, so a partner >= n is skipped.
__device__ __forceinline__ void xr_network(float *d, uint64_t *l, uint32_t n, uint32_t tid) {
  uint32_t n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (uint32_t size = 2; size <= n2; size <<= 1)
    for (uint32_t stride = size >> 1; stride; stride >>= 1) {
      const bool mirror = stride == (size >> 1);   // a stage's first step: i against size - 1 - i of its block
      for (uint32_t i = tid; i < (n2 >> 1); i += kRangeThreads) {
        const uint32_t lo = 2 * i - (i & (stride - 1));
        const uint32_t hi = mirror ? (lo | (size - 1)) - (lo & (stride - 1)) : lo + stride;
        if (hi >= n) continue;
        const float da = d[lo], db = d[hi];
        const uint64_t la = l[lo], lb = l[hi];
        if (db < da || (db == da && lb < la)) {
          d[lo] = db; l[lo] = lb;
          d[hi] = da; l[hi] = la;
        }
      }
      __syncthreads();   // (LDS and, for the long segments, the workgroup's own stores to device memory)
    }
}

// One workgroup per query: its segment sorted by (dist, label), in LDS up to kRangeSortLds entries, in place otherwise.
__global__ void __launch_bounds__(kRangeThreads) xr_sort_kernel(const uint64_t *offsets, uint32_t nq, uint64_t cap, uint64_t *out_labels,
                                                                 float *out_dists, uint32_t *over) {
  __shared__ uint64_t sl[kRangeSortLds];
  __shared__ float sd[kRangeSortLds];
  const uint32_t tid = threadIdx.x;
  if (offsets[nq] > cap) {
    if (tid == 0 && blockIdx.x == 0) atomicOr(over, 1u);
    return;
  }
  const uint64_t b = offsets[blockIdx.x], len64 = offsets[blockIdx.x + 1] - b;
  if (len64 < 2) return;
  const uint32_t len = (uint32_t)len64;   // (a segment holds at most n < 2^32 rows)
  float *d = out_dists + b;
  uint64_t *l = out_labels + b;
  if (len > kRangeSortLds) {
    xr_network(d, l, len, tid);
    return;
  }
  for (uint32_t i = tid; i < len; i += kRangeThreads) { sd[i] = d[i]; sl[i] = l[i]; }
  __syncthreads();
  xr_network(sd, sl, len, tid);
  for (uint32_t i = tid; i < len; i += kRangeThreads) { d[i] = sd[i]; l[i] = sl[i]; }
}

typedef void (*RangeKernel)(const RangeScan);
template <bool FILL>
static RangeKernel xr_pick(int fmt, bool l2, bool general) {
  return general            ? (l2 ? exact_range_general_kernel<METRIC_L2, FILL> : exact_range_general_kernel<METRIC_IP, FILL>)
         : fmt == ROWS_U8   ? (l2 ? exact_range_kernel_u8<METRIC_L2, FILL> : exact_range_kernel_u8<METRIC_IP, FILL>)
         : fmt == ROWS_I8   ? (l2 ? exact_range_kernel_i8<METRIC_L2, FILL> : exact_range_kernel_i8<METRIC_IP, FILL>)
         : fmt == ROWS_BF16 ? (l2 ? exact_range_kernel_bf16<METRIC_L2, FILL> : exact_range_kernel_bf16<METRIC_IP, FILL>)
         : fmt == ROWS_F8   ? (l2 ? exact_range_kernel_f8<METRIC_L2, FILL> : exact_range_kernel_f8<METRIC_IP, FILL>)
         : fmt == ROWS_F16  ? (l2 ? exact_range_kernel_f16<METRIC_L2, FILL> : exact_range_kernel_f16<METRIC_IP, FILL>)
                            : (l2 ? exact_range_kernel<METRIC_L2, FILL> : exact_range_kernel<METRIC_IP, FILL>);
}

const char *xr_kernel_name(uint32_t dim, int fmt) {
  return (dim & 15u)        ? "hs::exact_range_general_kernel"
         : fmt == ROWS_U8   ? "hs::exact_range_kernel_u8"
         : fmt == ROWS_I8   ? "hs::exact_range_kernel_i8"
         : fmt == ROWS_BF16 ? "hs::exact_range_kernel_bf16"
         : fmt == ROWS_F8   ? "hs::exact_range_kernel_f8"
         : fmt == ROWS_F16  ? "hs::exact_range_kernel_f16"
                            : "hs::exact_range_kernel";
}

// The scan of either pass: what both launch entries check and fill in.
template <bool FILL>
static hipError_t xr_launch_scan(const DevIndex &ix, const void *rows, int fmt, const RangeArgs &a, const FilterArgs *f, hipStream_t stream) {
  if (a.chunks == 0 || (a.rows_per_chunk & 255u)) return hipErrorInvalidValue;
  if ((uint64_t)a.chunks * a.rows_per_chunk < ix.n) return hipErrorInvalidValue;   // the chunks cover the rows
  const bool general = (ix.dim & 15u) != 0;
  if (general && fmt != ROWS_F32) return hipErrorInvalidValue;   // narrow rows exist for dim % 16 == 0 only
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  if (!a.queries || !a.radius || !a.counts || !a.bases || !a.out_offsets) return hipErrorInvalidDevicePointer;
  if (FILL && (!a.over || (a.cap && (!a.out_labels || !a.out_dists)))) return hipErrorInvalidDevicePointer;
  const RangeKernel kern = xr_pick<FILL>(fmt, ix.metric == METRIC_L2, general);
  const size_t lds = xr_lds_bytes(ix.dim);
  if (lds > 48 * 1024) {   // beyond the default limit of dynamic LDS: asked for by name
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  RangeScan sa{};
  sa.rows = rows; sa.labels = ix.labels; sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.queries = a.queries; sa.radius = a.radius; sa.order = a.order; sa.live = a.live;
  sa.counts = a.counts; sa.bases = a.bases; sa.total = a.out_offsets + a.nq;
  sa.cap = a.cap; sa.out_labels = a.out_labels; sa.out_dists = a.out_dists; sa.over = a.over;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = ix.dim; sa.nq = a.nq; sa.rows_per_chunk = a.rows_per_chunk;
  hipLaunchKernelGGL(kern, dim3((a.nq + kQT - 1) / kQT, a.chunks), dim3(kRangeThreads), lds, stream, sa);
  return hipGetLastError();
}

hipError_t launch_exact_range_count(const DevIndex &ix, const void *rows, int fmt, const RangeArgs &a, const FilterArgs *f, hipStream_t stream) {
  if (a.nq) {
    hipError_t e = xr_launch_scan<false>(ix, rows, fmt, a, f, stream);
    if (e != hipSuccess) return e;
  } else if (!a.out_offsets) return hipErrorInvalidDevicePointer;
  hipLaunchKernelGGL(xr_offsets_kernel, dim3(1), dim3(kRangeThreads), 0, stream, a.counts, a.nq, a.nq ? a.chunks : 1u, a.bases, a.out_offsets);
  return hipGetLastError();
}

hipError_t launch_exact_range_fill(const DevIndex &ix, const void *rows, int fmt, const RangeArgs &a, const FilterArgs *f, hipStream_t stream) {
  if (a.nq == 0) return hipSuccess;
  hipError_t e = xr_launch_scan<true>(ix, rows, fmt, a, f, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(xr_sort_kernel, dim3(a.nq), dim3(kRangeThreads), 0, stream, a.out_offsets, a.nq, a.cap, a.out_labels, a.out_dists, a.over);
  return hipGetLastError();
}

}  // namespace hs
