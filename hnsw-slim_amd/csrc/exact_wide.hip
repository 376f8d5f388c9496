// exact_wide.hip -- exact k-NN over the rows of a resident index for 64 < k <= 1024: exact_search.hip's candidates, distances and
// answer, with a selection scheme of its own.
//
// exact_search.hip keeps a sorted k-list per (wave, query) in LDS and inserts every admitted candidate serially on lane 0; that is
// 16 * 4 * 8 * k bytes and one shift per insertion, which is what stops it at k = 64.  Here:
//  * one list per (workgroup, query), shared by the four waves, in two parts: `kept`, KP = max(128, k rounded up to a power of two)
//    entries, sorted ascending and padded with +inf entries, and an unsorted append buffer of B = 256 entries.  The tile holds 8, 4
//    or 2 queries, so that two workgroups fit a CU (exact_wide_engine.hpp has the table);
//  * admission: a row is offered to query t if its bit is in t's admission word (filter row, less deleted rows and rows beyond n,
//    as exact_search.hip) and its distance is <= the threshold, the distance of kept[k - 1] (+inf until k are held).  The admitted
//    lanes of a pass are appended with one ballot, one prefix popcount per lane and one LDS atomic add per wave: no loop on lane 0;
//  * rounds: the workgroup walks its row chunk in rounds of 128 rows, one 32-row unit per wave (256 rows and 64 per wave for
//    dim % 16 != 0, one lane per row).  A round appends at most that many entries to a query's buffer, so at the round's start --
//    two barriers, the fill words are read between them, hence the same in every wave -- a buffer that could overflow is compacted;
//  * compaction: one wave per query, the queries of the tile side by side, synchronised by wave barriers only.  The wave pads the
//    buffer to a power of two with +inf entries, sorts it with a bitonic network, takes min(kept[KP - 1 - i], buf[i]) -- the KP
//    smallest of both as a bitonic sequence -- and finishes with one bitonic merge of KP.  The new threshold is written to LDS.
//    After the first k rows a query admits about k ln(n / k) rows in all, at most 128 per compaction: compactions are rare;
//  * row chunks exist only to fill the machine when there are few tiles (xw_plan).  With one chunk the scan writes labels, distances
//    and counts itself; otherwise it leaves a sorted run of k entries per (query, chunk) and xw_merge_kernel, one workgroup per query,
//    folds the runs into one list of KP in LDS by the same half-cleaner and bitonic merge.
// Determinism: (dist, label) is a total order on the candidates (labels are unique), every network sorts by it, and an entry that is
// not admitted or that a compaction drops has k smaller entries before it.  So kept[0 .. k) at the end is the k smallest of the
// candidate set whatever order waves and atomics appended in, and the same holds for the merge of the chunks' runs.
// Distances: exact_search.hip's passes, duplicated here -- four lanes per row, element 16 i + 4 sub + j reaches accumulator j of
// lane sub in step i, lane4_reduce; l2_general / ip_general for dim % 16 != 0 -- so an entry has the bits hs_index_exact_search gives.
// No matrix or dot-product instruction is involved.  The object is built without the packed fp32 instructions (Makefile).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bf_common.hpp"
#include "exact_wide_engine.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

static constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
static constexpr int kWideThreads = 64 * kWaves;

struct WideScan {
  const void *rows;          // fp32 rows or the narrow copy
  const uint64_t *labels;
  const uint8_t *deleted;    // null: the index has no delete marks
  const float *queries;
  const uint32_t *order;     // nullable
  BfEntry *partial;          // gridDim.y > 1: nq x gridDim.y runs of k entries
  uint64_t *out_labels;      // gridDim.y == 1: written by the scan
  float *out_dists;
  uint32_t *out_counts;      // nullable
  FilterArgs f;              // f.rows == null: no filter set
  uint32_t n, dim, nq, k, kp, qt, rows_per_chunk;
};

struct WideLds {
  float *q;            // qt x dim
  BfEntry *lists;      // qt x (kp + kWideBuf): kept, then the append buffer
  uint32_t *fill;      // qt: entries in the buffer
  float *thr;          // qt: the admission threshold
  uint32_t *slot_q;    // qt: the query a tile slot serves, kNoSlot beyond nq
  uint32_t *slot_f;    // qt: its filter row (0 without a filter set), kNoSlot = nothing is admitted
  uint32_t per;        // kp + kWideBuf
};

__device__ __forceinline__ BfEntry xw_pad() { return BfEntry{INFINITY, kNoSlot, ~0ull}; }   // after every candidate: a row index is < n
__device__ __forceinline__ bool xw_less(const BfEntry &a, const BfEntry &b) { return bf_less(a.d, a.label, b); }

// Add on a word of LDS as the DS instruction itself (wave_util.hpp lds_cas has the reason).
__device__ __forceinline__ uint32_t xw_lds_add(uint32_t *p, uint32_t v) {
  const uint32_t addr = (uint32_t)(uintptr_t)p;
  uint32_t old;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(v) : "memory");
  return old;
}

template <bool BLOCK>
__device__ __forceinline__ void xw_sync() {
  if (BLOCK) __syncthreads();
  else wave_sync();
}

// Bitonic network over A[0 .. n), n a power of two, by `nthreads` threads (a wave or the workgroup): a full ascending sort from
// first_size = 2, the ascending merge of a bitonic sequence from first_size = n.  Ends with a barrier of its group.
template <bool BLOCK>
__device__ __forceinline__ void xw_network(BfEntry *A, uint32_t n, uint32_t first_size, uint32_t id, uint32_t nthreads) {
  for (uint32_t size = first_size; size <= n; size <<= 1)
    for (uint32_t stride = size >> 1; stride; stride >>= 1) {
      for (uint32_t i = id; i < (n >> 1); i += nthreads) {
        const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const BfEntry a = A[lo], b = A[hi];
        const bool up = !(lo & size);   // (size == n: every pair ascends)
        if (xw_less(b, a) == up) { A[lo] = b; A[hi] = a; }
      }
      xw_sync<BLOCK>();
    }
}

// kept (ascending, kp entries) and other (ascending, m >= min(m, kp) entries used): the kp smallest of both, ascending, in kept.
template <bool BLOCK>
__device__ __forceinline__ void xw_fold(BfEntry *kept, uint32_t kp, const BfEntry *other, uint32_t m, uint32_t id, uint32_t nthreads) {
  const uint32_t lim = m < kp ? m : kp;
  for (uint32_t i = id; i < lim; i += nthreads) {
    const BfEntry b = other[i];
    if (xw_less(b, kept[kp - 1 - i])) kept[kp - 1 - i] = b;
  }
  xw_sync<BLOCK>();
  xw_network<BLOCK>(kept, kp, kp, id, nthreads);
}

// One wave empties a query's buffer (c entries, 1 <= c <= kWideBuf) into its kept list and renews the threshold.
__device__ __forceinline__ void xw_compact(BfEntry *kept, uint32_t kp, uint32_t k, uint32_t c, uint32_t *fill, float *thr, int lane) {
  BfEntry *buf = kept + kp;
  uint32_t n2 = 64;
  while (n2 < c) n2 <<= 1;
  for (uint32_t i = c + lane; i < n2; i += 64) buf[i] = xw_pad();
  wave_sync();
  xw_network<false>(buf, n2, 2, lane, 64);
  xw_fold<false>(kept, kp, buf, n2, lane, 64);
  if (lane == 0) {
    *fill = 0;
    *thr = kept[k - 1].d;
  }
}

// Stages the tile: which query and filter row each slot has, the queries, kept lists of +inf entries, empty buffers.
__device__ __forceinline__ WideLds xw_stage(const WideScan &a, unsigned char *smem, int tid) {
  WideLds s;
  const uint32_t qt = a.qt;
  s.per = a.kp + kWideBuf;
  s.q = reinterpret_cast<float *>(smem);
  s.lists = reinterpret_cast<BfEntry *>(smem + (((size_t)qt * a.dim * 4 + 15) & ~(size_t)15));
  s.fill = reinterpret_cast<uint32_t *>(s.lists + (size_t)qt * s.per);
  s.thr = reinterpret_cast<float *>(s.fill + qt);
  s.slot_q = s.fill + 2 * qt;
  s.slot_f = s.fill + 3 * qt;
  const uint32_t q0 = blockIdx.x * qt;
  if ((uint32_t)tid < qt) {
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
        else if (blockIdx.y == 0) atomicAdd(a.f.bad, 1u);   // once per query: its first row chunk
      }
    }
    s.slot_q[tid] = qi;
    s.slot_f[tid] = fi;
    s.fill[tid] = 0;
    s.thr[tid] = INFINITY;
  }
  for (uint32_t t = 0; t < qt; t++)
    for (uint32_t i = tid; i < a.kp; i += kWideThreads) s.lists[(size_t)t * s.per + i] = xw_pad();
  __syncthreads();
  for (uint32_t i = tid; i < qt * a.dim; i += kWideThreads) {
    const uint32_t t = i / a.dim, qi = s.slot_q[t];
    s.q[i] = qi != kNoSlot ? a.queries[(size_t)qi * a.dim + (i - t * a.dim)] : 0.f;
  }
  __syncthreads();
  return s;
}

// Admission word of unit u (rows 32 u .. 32 u + 31, 32 u < n) in lane t < qt for tile slot t (exact_search.hip exact_admit).
__device__ __forceinline__ uint32_t xw_admit(const WideScan &a, const WideLds &s, uint32_t u, int lane) {
  const uint32_t base = u * 32, left = a.n - base;
  uint32_t alive = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
  if (a.deleted) {
    const uint32_t idx = base + ((uint32_t)lane & 31u);
    const bool del = lane < 32 && idx < a.n && a.deleted[idx] != 0;
    alive &= ~(uint32_t)hs_ballot(del);
  }
  uint32_t w = 0;
  if ((uint32_t)lane < a.qt) {
    const uint32_t fi = s.slot_f[lane];
    if (fi != kNoSlot) w = a.f.rows ? a.f.rows[(size_t)fi * a.f.stride + u] : 0xFFFFFFFFu;
  }
  return w & alive;
}

// The lanes of mask m (not empty; the whole wave is here) append (d, row) to a query's buffer.
__device__ __forceinline__ void xw_append(unsigned long long m, float d, uint32_t row, const uint64_t *labels, BfEntry *buf, uint32_t *fill,
                                          int lane) {
  uint32_t base = 0;
  if (lane == 0) base = xw_lds_add(fill, (uint32_t)__popcll(m));
  base = uni(base);
  if ((m >> lane) & 1ull) {
    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    buf[pos] = BfEntry{d, row, labels ? labels[row] : (uint64_t)row};
  }
}

// Start of a round that appends at most `round_rows` entries per query: compacts every buffer that could overflow.  Called by the
// whole workgroup; the two barriers keep the fill words still while they are read.
__device__ __forceinline__ void xw_round_begin(const WideScan &a, const WideLds &s, uint32_t round_rows, int wave, int lane) {
  __syncthreads();
  uint32_t need = 0;
  for (uint32_t t = 0; t < a.qt; t++)
    if (s.fill[t] + round_rows > kWideBuf) need |= 1u << t;
  __syncthreads();
  if (!need) return;   // (workgroup uniform)
  for (uint32_t t = wave; t < a.qt; t += kWaves)
    if ((need >> t) & 1u) xw_compact(s.lists + (size_t)t * s.per, a.kp, a.k, uni(s.fill[t]), s.fill + t, s.thr + t, lane);
  __syncthreads();
}

// kept[0 .. k) of a finished list as the entry's outputs: ~0 / +inf from the first +inf entry on, which is the count.
__device__ __forceinline__ void xw_write_out(const BfEntry *kept, uint32_t k, uint64_t *labels, float *dists, uint32_t *count, int tid) {
  for (uint32_t i = tid; i < k; i += kWideThreads) {
    const BfEntry e = kept[i];
    const bool valid = e.row != kNoSlot;
    labels[i] = valid ? e.label : ~0ull;
    dists[i] = valid ? e.d : INFINITY;
    if (count) {
      if (valid && (i + 1 == k || kept[i + 1].row == kNoSlot)) *count = i + 1;
      if (i == 0 && !valid) *count = 0;
    }
  }
}

// End of the chunk: the buffers' rest goes into the kept lists, which leave as outputs (one chunk) or as runs for the merge.
__device__ __forceinline__ void xw_finish(const WideScan &a, const WideLds &s, int tid, int wave, int lane) {
  __syncthreads();
  for (uint32_t t = wave; t < a.qt; t += kWaves) {
    const uint32_t c = uni(s.fill[t]);
    if (c) xw_compact(s.lists + (size_t)t * s.per, a.kp, a.k, c, s.fill + t, s.thr + t, lane);
  }
  __syncthreads();
  for (uint32_t t = 0; t < a.qt; t++) {
    const uint32_t qi = s.slot_q[t];
    if (qi == kNoSlot) continue;
    const BfEntry *kept = s.lists + (size_t)t * s.per;
    if (gridDim.y == 1) {
      xw_write_out(kept, a.k, a.out_labels + (size_t)qi * a.k, a.out_dists + (size_t)qi * a.k, a.out_counts ? a.out_counts + qi : nullptr, tid);
    } else {
      BfEntry *dst = a.partial + ((size_t)qi * gridDim.y + blockIdx.y) * a.k;
      for (uint32_t i = tid; i < a.k; i += kWideThreads) dst[i] = kept[i];
    }
  }
}

// One 32-row unit of a wave, dim % 16 == 0: 4 lanes per row, 16 rows per pass, two passes (exact_search.hip exact_scan_body).
template <int METRIC, typename ROW, int QT>
__device__ __forceinline__ void xw_unit(const WideScan &a, const WideLds &s, uint32_t u, uint32_t r0, int lane) {
  const int sub = lane & 3, grp = lane >> 2;
  const float *q = s.q;
  const uint32_t dim = a.dim, steps = dim >> 4;
  const uint32_t w = xw_admit(a, s, u, lane);
  uint32_t aw[QT], un = 0;
#pragma unroll
  for (int t = 0; t < QT; t++) {
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
    float acc[QT][4];
#pragma unroll
    for (int t = 0; t < QT; t++) acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f;
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
            for (int t = 0; t < QT; t++) {
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
        for (int t = 0; t < QT; t++) {
          const float4 qv = *reinterpret_cast<const float4 *>(q + (size_t)t * dim + st * 16 + sub * 4);
          step4<METRIC>(acc[t], qv, xv);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < QT; t++) {
      bool owner;
      const float d = lane4_reduce<METRIC>(acc[t], sub, owner);
      if (!((aw[t] >> h) & 0xFFFFu)) continue;   // (wave uniform)
      const bool adm = (aw[t] >> (h + grp)) & 1u;
      const unsigned long long m = hs_ballot(adm && owner && d <= s.thr[t]);   // bruteforce.h:120 `dist <= lastdist`
      if (m) xw_append(m, d, row, a.labels, s.lists + (size_t)t * s.per + a.kp, s.fill + t, lane);
    }
  }
}

template <int METRIC, typename ROW, int QT>
__device__ __forceinline__ void xw_scan_body(const WideScan &a, unsigned char *smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WideLds s = xw_stage(a, smem, tid);
  const uint32_t r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint32_t rb = r0; rb < r1; rb += 32 * kWaves) {
    xw_round_begin(a, s, 32 * kWaves, wave, lane);
    const uint32_t u = (rb >> 5) + wave;
    if (u * 32 < r1) xw_unit<METRIC, ROW, QT>(a, s, u, r0, lane);
  }
  xw_finish(a, s, tid, wave, lane);
}

#define HS_WIDE_KERNEL(NAME, ROW)                                                                 \
  template <int METRIC, int QT>                                                                   \
  __global__ void __launch_bounds__(kWideThreads) NAME(const WideScan a) {                        \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                          \
    xw_scan_body<METRIC, ROW, QT>(a, smem);                                                       \
  }
HS_WIDE_KERNEL(exact_wide_kernel, float)
HS_WIDE_KERNEL(exact_wide_kernel_u8, uint8_t)
HS_WIDE_KERNEL(exact_wide_kernel_i8, int8_t)
HS_WIDE_KERNEL(exact_wide_kernel_f16, _Float16)
HS_WIDE_KERNEL(exact_wide_kernel_bf16, hs_bf16)
HS_WIDE_KERNEL(exact_wide_kernel_f8, hs_f8)
#undef HS_WIDE_KERNEL

// dim % 16 != 0 (fp32 rows only): dist_recipe.hpp's l2_general / ip_general, one lane per row, 64 rows = two units per wave and
// round, as exact_search.hip's exact_scan_general_kernel.  A round may fill a whole buffer, so every buffer that holds anything is
// compacted at the round's start.
template <int METRIC>
__global__ void __launch_bounds__(kWideThreads) exact_wide_general_kernel(const WideScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WideLds s = xw_stage(a, smem, tid);
  const uint32_t dim = a.dim;
  const uint32_t r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint32_t rb = r0; rb < r1; rb += 64 * kWaves) {
    xw_round_begin(a, s, 64 * kWaves, wave, lane);
    const uint32_t wb = rb + wave * 64;
    if (wb >= r1) continue;   // (the loop condition is the workgroup's: every wave comes back to the barriers)
    const uint32_t w0 = xw_admit(a, s, wb >> 5, lane);
    const uint32_t w1 = wb + 32 < r1 ? xw_admit(a, s, (wb >> 5) + 1, lane) : 0u;
    if (!hs_ballot((uint32_t)lane < a.qt && (w0 | w1) != 0)) continue;   // no slot admits a row of these two units
    const uint32_t row = wb + lane;
    const float *x = static_cast<const float *>(a.rows) + (size_t)(row < r1 ? row : r0) * dim;
#pragma unroll 1
    for (uint32_t t = 0; t < a.qt; t++) {
      const uint32_t lo = __builtin_amdgcn_readlane(w0, t), hi = __builtin_amdgcn_readlane(w1, t);
      const unsigned long long at = ((unsigned long long)hi << 32) | lo;
      if (!at) continue;   // (wave uniform)
      const float d = METRIC == METRIC_L2 ? l2_general(s.q + (size_t)t * dim, x, dim) : ip_general(s.q + (size_t)t * dim, x, dim);
      const bool adm = (at >> lane) & 1ull;
      const unsigned long long m = hs_ballot(adm && d <= s.thr[t]);
      if (m) xw_append(m, d, row, a.labels, s.lists + (size_t)t * s.per + a.kp, s.fill + t, lane);
    }
  }
  xw_finish(a, s, tid, wave, lane);
}

// One workgroup per query: the sorted runs of its row chunks (k entries each, +inf entries last) folded into one list of KP.
__global__ void __launch_bounds__(kWideThreads) xw_merge_kernel(const BfEntry *partial, uint32_t chunks, uint32_t k, uint32_t kp,
                                                                uint64_t *out_labels, float *out_dists, uint32_t *out_counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  BfEntry *acc = reinterpret_cast<BfEntry *>(smem), *in = acc + kp;
  const int tid = threadIdx.x;
  const uint32_t qi = blockIdx.x;
  const BfEntry *run = partial + (size_t)qi * chunks * k;
  for (uint32_t i = tid; i < kp; i += kWideThreads) acc[i] = i < k ? run[i] : xw_pad();
  for (uint32_t c = 1; c < chunks; c++) {
    run += k;
    for (uint32_t i = tid; i < kp; i += kWideThreads) in[i] = i < k ? run[i] : xw_pad();
    __syncthreads();
    xw_fold<true>(acc, kp, in, kp, tid, kWideThreads);
  }
  __syncthreads();
  xw_write_out(acc, k, out_labels + (size_t)qi * k, out_dists + (size_t)qi * k, out_counts ? out_counts + qi : nullptr, tid);
}

typedef void (*WideKernel)(const WideScan);
template <int QT>
static WideKernel xw_pick(int fmt, bool l2) {
  return fmt == ROWS_U8     ? (l2 ? exact_wide_kernel_u8<METRIC_L2, QT> : exact_wide_kernel_u8<METRIC_IP, QT>)
         : fmt == ROWS_I8   ? (l2 ? exact_wide_kernel_i8<METRIC_L2, QT> : exact_wide_kernel_i8<METRIC_IP, QT>)
         : fmt == ROWS_BF16 ? (l2 ? exact_wide_kernel_bf16<METRIC_L2, QT> : exact_wide_kernel_bf16<METRIC_IP, QT>)
         : fmt == ROWS_F8   ? (l2 ? exact_wide_kernel_f8<METRIC_L2, QT> : exact_wide_kernel_f8<METRIC_IP, QT>)
         : fmt == ROWS_F16  ? (l2 ? exact_wide_kernel_f16<METRIC_L2, QT> : exact_wide_kernel_f16<METRIC_IP, QT>)
                            : (l2 ? exact_wide_kernel<METRIC_L2, QT> : exact_wide_kernel<METRIC_IP, QT>);
}

const char *xw_kernel_name(uint32_t dim, int fmt) {
  return (dim & 15u)        ? "hs::exact_wide_general_kernel"
         : fmt == ROWS_U8   ? "hs::exact_wide_kernel_u8"
         : fmt == ROWS_I8   ? "hs::exact_wide_kernel_i8"
         : fmt == ROWS_BF16 ? "hs::exact_wide_kernel_bf16"
         : fmt == ROWS_F8   ? "hs::exact_wide_kernel_f8"
         : fmt == ROWS_F16  ? "hs::exact_wide_kernel_f16"
                            : "hs::exact_wide_kernel";
}

hipError_t launch_exact_wide(const DevIndex &ix, const void *rows, int fmt, const ExactArgs &a, const FilterArgs *f, hipStream_t stream) {
  if (a.k <= 64 || a.k > kWideMaxK || a.grid_x == 0 || (a.rows_per_block & 255u)) return hipErrorInvalidValue;
  if ((uint64_t)a.grid_x * a.rows_per_block < ix.n) return hipErrorInvalidValue;   // the chunks cover the rows
  const uint32_t qt = xw_tile(ix.dim, a.k);
  if (!qt) return hipErrorInvalidValue;   // not even two queries fit the CU's LDS
  const bool general = (ix.dim & 15u) != 0;
  if (general && fmt != ROWS_F32) return hipErrorInvalidValue;   // narrow rows exist for dim % 16 == 0 only
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  if (a.grid_x > 1 && !a.partial) return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2;
  const WideKernel kern = general   ? (l2 ? exact_wide_general_kernel<METRIC_L2> : exact_wide_general_kernel<METRIC_IP>)
                          : qt == 8 ? xw_pick<8>(fmt, l2)
                          : qt == 4 ? xw_pick<4>(fmt, l2)
                                    : xw_pick<2>(fmt, l2);
  const size_t lds = xw_lds_bytes(ix.dim, a.k, qt);
  if (lds > 48 * 1024) {   // beyond the default limit of dynamic LDS: asked for by name
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  WideScan sa{};
  sa.rows = rows; sa.labels = ix.labels; sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.queries = a.queries; sa.order = a.order; sa.partial = static_cast<BfEntry *>(a.partial);
  sa.out_labels = a.out_labels; sa.out_dists = a.out_dists; sa.out_counts = a.out_counts;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = ix.dim; sa.nq = a.nq; sa.k = a.k; sa.kp = xw_kp(a.k); sa.qt = qt; sa.rows_per_chunk = a.rows_per_block;
  const dim3 grid((a.nq + qt - 1) / qt, a.grid_x);
  hipLaunchKernelGGL(kern, grid, dim3(kWideThreads), lds, stream, sa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.grid_x == 1) return e;
  hipLaunchKernelGGL(xw_merge_kernel, dim3(a.nq), dim3(kWideThreads), 2 * (size_t)sa.kp * sizeof(BfEntry), stream, sa.partial, a.grid_x, a.k, sa.kp,
                     a.out_labels, a.out_dists, a.out_counts);
  return hipGetLastError();
}

}  // namespace hs
