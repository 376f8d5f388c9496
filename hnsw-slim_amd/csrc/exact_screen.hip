// exact_screen.hip -- exact k-NN over a resident index's rows in three steps: a screen on the matrix cores that rules
// rows out by a cheaper distance with a proven margin, a re-rank of the few survivors in the reference's arithmetic, and, for the
// queries the screen cannot decide, the scan of exact_search.hip.  The answer is that scan's, bit for bit.
//
// Why that holds: a query's answer is the set of its k smallest (dist, label) pairs, whatever the scan order.  For an admitted row the
// screen computes a (L2: |q|^2 + |x|^2 - 2 q.x, IP: 1 - q.x; the dot product by v_mfma_f32_32x32x2f32) and e = exact_screen_margin
// with |a - r| <= e for the recipe's distance r, so r lies in [lo, hi] = [a - e, a + e].  U = the k-th smallest hi over any >= k
// admitted rows bounds the k-th smallest r from above; every row of the answer, and every row that ties with its last entry, has
// lo <= U.  Keeping the rows with lo <= U is keeping a superset; the recipe over the superset and the k smallest (dist, label) of it
// is the answer.  U only falls as rows are seen: a running U per row chunk is valid, the U of the merge is tighter.
//
// xs_norms_kernel   |x|^2 per row in the format the index holds, |q|^2 per query (any summation order satisfies the bound).
// xs_screen_kernel  a workgroup of 4 waves, a tile of 64 queries, a chunk of rows.  The tile sits in LDS as fp32 in operand layout:
//                   one 16-byte read gives a lane the query values of four MFMA steps.  Wave (b, p) owns the 32 queries of half b
//                   and the 32-row units of parity p: one 32 x 32 accumulator block per unit, rows straight from global memory into
//                   the other operand (16 bytes of fp32, 4 of u8 / i8 / fp8, 8 of fp16 / bf16 per lane and four steps, the next load in flight under the
//                   MFMAs).  The k index may be permuted freely as long as both operands agree, so the narrow copy is read in the
//                   order it is stored and the tile is staged in that order.  Epilogue per accumulator element: a, e, lo, hi,
//                   admission as exact_search.hip's, lo <= U_q; the few survivors go through a ballot into the (parity, query)
//                   list in LDS -- sorted by hi, capacity k + 16, U_q its k-th hi.  No list is shared between waves.  A tile too long
//                   for the LDS goes through it in slices of 128 positions, each wave carrying four accumulator blocks across them.
// xs_rerank_kernel  one wave per query: gathers the chunks' lists, finds the final U (k-th smallest hi, bisection on the keys), keeps
//                   lo <= U, computes r four lanes per row with the scan's own step4 / lane4_reduce, ranks by (dist, label).
// A query is flagged -- and left to the scan, which is enqueued behind the re-rank and finds its queries on the device -- when an
// admitted row's interval is not finite or a list overflows, in a chunk or at the merge.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bf_common.hpp"
#include "exact_screen_engine.hpp"
#include "exact_screen_margin.hpp"
#include "exact_screen_rows.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

static constexpr uint32_t kXsMerge = 2048;   // entries the re-rank gathers per query
static constexpr uint32_t kXsKeep = 512;     // rows it re-ranks per query

// ---- norms -------------------------------------------------------------------------------------------------------------------
// 16 lanes per vector, 16 vectors per workgroup; a narrow row is summed in the order it is stored.
template <typename ROW>
__global__ void __launch_bounds__(256) xs_norms_kernel(const ROW *v, uint32_t n, uint32_t dim, float *out) {
  const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  float s = 0.f;
  if (r < n) {
    const ROW *x = v + (size_t)r * dim;
    for (uint32_t i = l; i < dim; i += 16) {
      const float e = (float)x[i];
      s = __builtin_fmaf(e, e, s);
    }
  }
  s += __shfl_xor(s, 8, 16);
  s += __shfl_xor(s, 4, 16);
  s += __shfl_xor(s, 2, 16);
  s += __shfl_xor(s, 1, 16);
  if (r < n && l == 0) out[r] = s;
}

// clears what a launch group accumulates (no memset node: the sequence may be captured)
__global__ void __launch_bounds__(256) xs_init_kernel(uint32_t *state, uint32_t *qflag, uint32_t *fb_order, uint32_t nq, uint32_t first) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nq) { qflag[i] = 0; fb_order[i] = kXsNoSlot; }
  if (i == 0) state[0] = 0;
  if (first && i >= 1 && i < kXsStateWords) state[i] = 0;   // (the first workgroup has 256 threads)
}

// ---- screen ------------------------------------------------------------------------------------------------------------------
struct XsScan {
  const void *rows;
  const uint8_t *deleted;
  const float *queries, *xn, *qn;
  const uint32_t *order;
  unsigned char *cand;
  uint32_t *qflag;
  FilterArgs f;
  uint32_t n, dim, nq, k, cap, rows_per_block, slice;
};

// (the row operand in stored order -- XsChunk -- and the tile's staging -- xs_stage: exact_screen_rows.hpp)
// NU: 32-row units a wave carries at a time, one accumulator block each.  A tile that fits the LDS whole (a.slice == dim) is staged
// once and NU is 1.  A longer one is staged in slices of a.slice positions: the workgroup then advances in steps of 2 NU units per
// parity pair, and for every slice stages it (two barriers) and lets each wave add the slice's products to its NU blocks, so a
// slice is fetched once per 64 NU rows.
template <int METRIC, typename ROW, int NU>
__device__ __forceinline__ void xs_screen_body(const XsScan &a, unsigned char *smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = wave & 1, p = wave >> 1, j = lane & 31, h = lane >> 5;
  const uint32_t dim = a.dim, k = a.k, cap = a.cap, slice = a.slice;
  float *qL = reinterpret_cast<float *>(smem);                       // (slice / 8) x 2 x 64 x 4
  float *qn2 = qL + (size_t)kXsTile * slice;                         // 64
  uint32_t *slot_q = reinterpret_cast<uint32_t *>(qn2 + kXsTile);    // 64
  uint32_t *slot_f = slot_q + kXsTile;                               // 64
  uint32_t *sizes = slot_f + kXsTile;                                // 2 x 64
  float *ub = reinterpret_cast<float *>(sizes + 2 * kXsTile);        // 2 x 64
  uint32_t *lflag = reinterpret_cast<uint32_t *>(ub + 2 * kXsTile);  // 2 x 64
  XsCand *lists = reinterpret_cast<XsCand *>(lflag + 2 * kXsTile);   // 2 x 64 x cap
  const uint32_t q0 = blockIdx.y * kXsTile;
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
        else if (blockIdx.x == 0) atomicAdd(a.f.bad, 1u);   // once per query: its first row chunk
      }
    }
    slot_q[tid] = qi;
    slot_f[tid] = fi;
    qn2[tid] = qi != kXsNoSlot ? a.qn[qi] : 0.f;
  }
  if (tid < (int)(2 * kXsTile)) { sizes[tid] = 0; ub[tid] = INFINITY; lflag[tid] = 0; }
  __syncthreads();
  const bool whole = slice >= dim;
  if (whole) {
    xs_stage<ROW>(qL, slot_q, a.queries, dim, 0, dim, tid);
    __syncthreads();
  }

  const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const float4 *qA = reinterpret_cast<const float4 *>(qL) + h * kXsTile + 32 * b + j;   // + 128 per chunk of 8 positions
  const uint32_t lbase = p * kXsTile + 32 * b;   // this wave's lists: lbase + local slot
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
    // element v of lane (j, h): query slot 8 (v / 4) + 4 h + v % 4 of the half against row j of the unit
#pragma unroll
    for (int i = 0; i < NU; i++) {
      if (!act[i]) continue;
      const uint32_t base = (ug + p + 2 * i) * 32, row = base + j;
      const float xnl = row < a.n ? a.xn[row] : 0.f;
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const uint32_t tl = 8u * (v >> 2) + 4u * h + (v & 3);
        const uint32_t awv = (uint32_t)__shfl((int)w[i], (int)tl);
        const bool adm = (awv >> j) & 1u;
        const float qq = qn2[32 * b + tl];
        const float dot = acc[i][v];
        const float av = METRIC == METRIC_L2 ? (qq + xnl) - 2.f * dot : 1.f - dot;
        const float e = exact_screen_margin(METRIC == METRIC_IP, dim, qq, xnl);
        const float lo = av - e, hi = av + e;
        const bool fin = (lo - lo == 0.f) && (hi - hi == 0.f);
        if (adm && !fin) lflag[lbase + tl] = 1;   // (several lanes may write the same 1)
        unsigned long long m = hs_ballot(adm && fin && lo <= ub[lbase + tl]);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float hj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(hi), l));
          const float lj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lo), l));
          if (lane == 0) {
            const uint32_t li = lbase + 8u * (v >> 2) + 4u * ((uint32_t)l >> 5) + (v & 3);
            xs_insert(lists + (size_t)li * cap, sizes + li, ub + li, lflag + li, k, cap, hj, lj, base + ((uint32_t)l & 31u));
          }
          wave_sync();
        }
      }
    }
  }
  wave_sync();
  // this wave's 32 lists, at the position of the query a slot serves
  const uint32_t nruns = gridDim.x * 2, run = blockIdx.x * 2 + p;
  XsCand *out = reinterpret_cast<XsCand *>(a.cand);
  uint32_t *hdr = reinterpret_cast<uint32_t *>(a.cand + xs_hdr_offset(a.nq, nruns, cap));
  for (uint32_t tl = 0; tl < 32; tl++) {
    const uint32_t qi = slot_q[32 * b + tl], li = lbase + tl;
    if (qi == kXsNoSlot) continue;
    const uint32_t sz = sizes[li];
    const size_t at = (size_t)qi * nruns + run;
    for (uint32_t i = lane; i < sz; i += 64) out[at * cap + i] = lists[(size_t)li * cap + i];
    if (lane == 0) {
      hdr[at] = sz;
      if (lflag[li]) a.qflag[qi] = 1;
    }
  }
}

template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, float, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel_u8(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, uint8_t, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel_i8(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, int8_t, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel_bf16(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, hs_bf16, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel_f8(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, hs_f8, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xs_screen_kernel_f16(const XsScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_screen_body<METRIC, _Float16, NU>(a, smem);
}

// ---- re-rank -----------------------------------------------------------------------------------------------------------------
struct XsRerank {
  const void *rows;
  const uint64_t *labels;
  const float *queries;
  const unsigned char *cand;
  const uint32_t *qflag;
  uint32_t *state, *fb_order;
  uint64_t *out_labels;
  float *out_dists;
  uint32_t *out_counts;
  uint32_t dim, nq, k, cap, nruns;
};

// order-preserving key of a float, and back
__device__ __forceinline__ uint32_t xs_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float xs_unkey(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? key & 0x7FFFFFFFu : ~key); }
__device__ __forceinline__ uint32_t xs_wave_sum(uint32_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
  return v;
}

// (the recipe's distance of one pair, four lanes per row -- xs_recipe_dist: exact_screen_rows.hpp)
template <int METRIC, typename ROW>
__device__ __forceinline__ void xs_rerank_body(const XsRerank &a, float *q) {
  __shared__ float c_hi[kXsMerge], c_lo[kXsMerge];
  __shared__ uint32_t c_row[kXsMerge];
  __shared__ float k_d[kXsKeep];
  __shared__ uint64_t k_l[kXsKeep];
  const uint32_t qi = blockIdx.x, k = a.k, cap = a.cap, nruns = a.nruns, dim = a.dim;
  const int lane = threadIdx.x, sub = lane & 3, grp = lane >> 2;
  const XsCand *ent = reinterpret_cast<const XsCand *>(a.cand) + (size_t)qi * nruns * cap;
  const uint32_t *hdr = reinterpret_cast<const uint32_t *>(a.cand + xs_hdr_offset(a.nq, nruns, cap)) + (size_t)qi * nruns;
  bool flagged = a.qflag[qi] != 0;   // (wave uniform)
  uint32_t m = 0, kc = 0;
  if (!flagged) {
    // a first bound from the chunks that hold k entries, then every entry it does not rule out
    float u0 = INFINITY;
    for (uint32_t r = lane; r < nruns; r += 64)
      if (hdr[r] >= k) u0 = fminf(u0, ent[(size_t)r * cap + k - 1].hi);
    u0 = wave_min_f32<true>(u0);
    for (uint32_t r = 0; r < nruns; r++) {
      const uint32_t sz = min(hdr[r], cap);
      for (uint32_t i0 = 0; i0 < sz; i0 += 64) {
        const uint32_t i = i0 + lane;
        XsCand e{0.f, 0.f, 0u};
        if (i < sz) e = ent[(size_t)r * cap + i];
        const bool keep = i < sz && e.lo <= u0;
        const unsigned long long mask = hs_ballot(keep);
        const uint32_t pos = m + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (keep && pos < kXsMerge) { c_hi[pos] = e.hi; c_lo[pos] = e.lo; c_row[pos] = e.row; }
        m += (uint32_t)__popcll(mask);
      }
    }
    wave_sync();
    flagged = m > kXsMerge;
  }
  if (!flagged) {
    // the final bound: the k-th smallest hi, bit by bit -- the largest key with fewer than k keys below it
    float U = INFINITY;
    if (m >= k) {
      uint32_t key = 0;
      for (int bit = 31; bit >= 0; bit--) {
        const uint32_t tryk = key | (1u << bit);
        uint32_t c = 0;
        for (uint32_t i = lane; i < m; i += 64) c += xs_key(c_hi[i]) < tryk;
        if (xs_wave_sum(c) < k) key = tryk;
      }
      U = xs_unkey(key);
    }
    // keep lo <= U, in place (every position written lies at or below the ones just read)
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
      const uint32_t i = i0 + lane;
      const float lo = i < m ? c_lo[i] : 0.f;
      const uint32_t row = i < m ? c_row[i] : 0u;
      wave_sync();
      const bool keep = i < m && lo <= U;
      const unsigned long long mask = hs_ballot(keep);
      if (keep) c_row[kc + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = row;
      kc += (uint32_t)__popcll(mask);
      wave_sync();
    }
    flagged = kc > kXsKeep;
  }
  if (flagged) {   // the scan behind this kernel serves the query; nothing is written here
    if (lane == 0) {
      a.fb_order[atomicAdd(a.state + 0, 1u)] = qi;
      atomicAdd(a.state + 1, 1u);
    }
    return;
  }
  for (uint32_t i = lane; i < dim; i += 64) q[i] = a.queries[(size_t)qi * dim + i];
  wave_sync();
  for (uint32_t e0 = 0; e0 < kc; e0 += 16) {
    const uint32_t idx = e0 + grp;
    const bool act = idx < kc;
    const uint32_t row = c_row[act ? idx : 0];   // idle groups repeat the first row and discard
    bool owner;
    const float d = xs_recipe_dist<METRIC, ROW>(q, a.rows, (size_t)row * dim, dim, sub, owner);
    if (act && owner) { k_d[idx] = d; k_l[idx] = a.labels[row]; }
  }
  wave_sync();
  // position = the number of kept rows below it under (dist, label), the list position breaking what is left
  for (uint32_t e = lane; e < kc; e += 64) {
    const float de = k_d[e];
    const uint64_t le = k_l[e];
    uint32_t rank = 0;
    for (uint32_t f = 0; f < kc; f++) {
      const float df = k_d[f];
      const uint64_t lf = k_l[f];
      rank += df < de || (df == de && (lf < le || (lf == le && f < e)));
    }
    if (rank < k) { a.out_labels[(size_t)qi * k + rank] = le; a.out_dists[(size_t)qi * k + rank] = de; }
  }
  const uint32_t found = min(k, kc);
  for (uint32_t i = found + lane; i < k; i += 64) { a.out_labels[(size_t)qi * k + i] = ~0ull; a.out_dists[(size_t)qi * k + i] = INFINITY; }
  if (lane == 0) {
    if (a.out_counts) a.out_counts[qi] = found;
    atomicAdd(reinterpret_cast<unsigned long long *>(a.state + 2), (unsigned long long)kc);
  }
}

template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, float>(a, reinterpret_cast<float *>(smem));
}
template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel_u8(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, uint8_t>(a, reinterpret_cast<float *>(smem));
}
template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel_i8(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, int8_t>(a, reinterpret_cast<float *>(smem));
}
template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel_bf16(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, hs_bf16>(a, reinterpret_cast<float *>(smem));
}
template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel_f8(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, hs_f8>(a, reinterpret_cast<float *>(smem));
}
template <int METRIC>
__global__ void __launch_bounds__(64) xs_rerank_kernel_f16(const XsRerank a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xs_rerank_body<METRIC, _Float16>(a, reinterpret_cast<float *>(smem));
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kXsSlice = 128;   // positions per slice of a tile that does not fit whole
static constexpr int kXsSliceUnits = 4;     // units a wave carries per slice (NU)
static size_t xs_lds_for(uint32_t slice, uint32_t k) {
  return (size_t)kXsTile * slice * 4 + 3 * kXsTile * 4 + 3 * 2 * kXsTile * 4 + (size_t)2 * kXsTile * xs_cap(k) * sizeof(XsCand);
}
uint32_t xs_slice(uint32_t dim, uint32_t k) { return xs_lds_for(dim, k) <= 160 * 1024 ? dim : kXsSlice; }
size_t xs_screen_lds_bytes(uint32_t dim, uint32_t k) { return xs_lds_for(xs_slice(dim, k), k); }
bool xs_supported(uint32_t dim, uint32_t k) { return dim != 0 && (dim & 15u) == 0 && dim <= 4096 && k >= 1 && k <= 64; }
size_t xs_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t *grid_x, uint32_t *rows_per_block) {
  // enough workgroups to fill the chip for few queries; a chunk of at least 512 rows, so that a list's own bound means something
  const uint32_t tiles = (nq + kXsTile - 1) / kXsTile;
  uint32_t gx = (1024 + tiles - 1) / tiles;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  uint32_t rpb = ((n + gx - 1) / gx + 63) / 64 * 64;
  if (rpb < 512) rpb = 512;
  gx = (n + rpb - 1) / rpb;
  if (gx == 0) gx = 1;
  *grid_x = gx;
  *rows_per_block = rpb;
  return xs_hdr_offset(nq, gx * 2, xs_cap(k)) + (size_t)nq * gx * 2 * sizeof(uint32_t);
}
const char *xs_kernel_name(int fmt) {
  return fmt == ROWS_U8 ? "hs::xs_screen_kernel_u8" : fmt == ROWS_I8 ? "hs::xs_screen_kernel_i8" : fmt == ROWS_BF16 ? "hs::xs_screen_kernel_bf16" : fmt == ROWS_F8 ? "hs::xs_screen_kernel_f8" : fmt == ROWS_F16 ? "hs::xs_screen_kernel_f16" : "hs::xs_screen_kernel";
}

hipError_t launch_exact_screen_norms(const DevIndex &ix, const void *rows, int fmt, float *xnorm2, hipStream_t stream) {
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!ix.n) return hipSuccess;
  if (!rows) return hipErrorInvalidDevicePointer;
  const dim3 g((ix.n + 15) / 16);
  if (fmt == ROWS_U8) hipLaunchKernelGGL(xs_norms_kernel<uint8_t>, g, dim3(256), 0, stream, static_cast<const uint8_t *>(rows), ix.n, ix.dim, xnorm2);
  else if (fmt == ROWS_I8) hipLaunchKernelGGL(xs_norms_kernel<int8_t>, g, dim3(256), 0, stream, static_cast<const int8_t *>(rows), ix.n, ix.dim, xnorm2);
  else if (fmt == ROWS_BF16) hipLaunchKernelGGL(xs_norms_kernel<hs_bf16>, g, dim3(256), 0, stream, static_cast<const hs_bf16 *>(rows), ix.n, ix.dim, xnorm2);
  else if (fmt == ROWS_F8) hipLaunchKernelGGL(xs_norms_kernel<hs_f8>, g, dim3(256), 0, stream, static_cast<const hs_f8 *>(rows), ix.n, ix.dim, xnorm2);
  else if (fmt == ROWS_F16) hipLaunchKernelGGL(xs_norms_kernel<_Float16>, g, dim3(256), 0, stream, static_cast<const _Float16 *>(rows), ix.n, ix.dim, xnorm2);
  else hipLaunchKernelGGL(xs_norms_kernel<float>, g, dim3(256), 0, stream, static_cast<const float *>(rows), ix.n, ix.dim, xnorm2);
  return hipGetLastError();
}

hipError_t launch_exact_screen_qnorms(const float *queries, uint32_t nq, uint32_t dim, float *qnorm2, hipStream_t stream) {
  hipLaunchKernelGGL(xs_norms_kernel<float>, dim3((nq + 15) / 16), dim3(256), 0, stream, queries, nq, dim, qnorm2);
  return hipGetLastError();
}

hipError_t launch_exact_screen(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const FilterArgs *f, hipStream_t stream) {
  const uint32_t dim = ix.dim, nq = a.x.nq, k = a.x.k;
  if (!xs_supported(dim, k) || nq == 0) return hipErrorInvalidValue;
  if (fmt == ROWS_F32) rows = ix.vec;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2;
  hipError_t e;
  if ((e = launch_exact_screen_init(a, stream)) != hipSuccess) return e;
  if ((e = launch_exact_screen_qnorms(a.x.queries, nq, dim, a.qnorm2, stream)) != hipSuccess) return e;

  const uint32_t slice = xs_slice(dim, k);
  void (*screen)(const XsScan);
#define HS_XS_PICK(NU)                                                                                                       \
  screen = fmt == ROWS_U8    ? (l2 ? xs_screen_kernel_u8<METRIC_L2, NU> : xs_screen_kernel_u8<METRIC_IP, NU>)                  \
           : fmt == ROWS_I8  ? (l2 ? xs_screen_kernel_i8<METRIC_L2, NU> : xs_screen_kernel_i8<METRIC_IP, NU>)                  \
           : fmt == ROWS_BF16 ? (l2 ? xs_screen_kernel_bf16<METRIC_L2, NU> : xs_screen_kernel_bf16<METRIC_IP, NU>)             \
           : fmt == ROWS_F8  ? (l2 ? xs_screen_kernel_f8<METRIC_L2, NU> : xs_screen_kernel_f8<METRIC_IP, NU>)                  \
           : fmt == ROWS_F16 ? (l2 ? xs_screen_kernel_f16<METRIC_L2, NU> : xs_screen_kernel_f16<METRIC_IP, NU>)                \
                             : (l2 ? xs_screen_kernel<METRIC_L2, NU> : xs_screen_kernel<METRIC_IP, NU>)
  if (slice >= dim) HS_XS_PICK(1);
  else HS_XS_PICK(kXsSliceUnits);
#undef HS_XS_PICK
  const size_t lds = xs_screen_lds_bytes(dim, k);
  if (lds > 48 * 1024) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(screen), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  XsScan sa{};
  sa.rows = rows; sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.queries = a.x.queries; sa.xn = a.xnorm2; sa.qn = a.qnorm2; sa.order = a.x.order;
  sa.cand = static_cast<unsigned char *>(a.cand); sa.qflag = a.qflag;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = dim; sa.nq = nq; sa.k = k; sa.cap = xs_cap(k); sa.rows_per_block = a.rows_per_block; sa.slice = slice;
  hipLaunchKernelGGL(screen, dim3(a.grid_x, (nq + kXsTile - 1) / kXsTile), dim3(256), lds, stream, sa);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_exact_screen_finish(ix, rows, fmt, a, f, stream);
}

hipError_t launch_exact_screen_init(const ScreenArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(xs_init_kernel, dim3((a.x.nq + 255) / 256), dim3(256), 0, stream, a.state, a.qflag, a.fb_order, a.x.nq, a.first_group ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_exact_screen_finish(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const FilterArgs *f, hipStream_t stream) {
  const uint32_t dim = ix.dim, nq = a.x.nq, k = a.x.k;
  const bool l2 = ix.metric == METRIC_L2;
  hipError_t e;
  void (*rerank)(const XsRerank) = fmt == ROWS_U8    ? (l2 ? xs_rerank_kernel_u8<METRIC_L2> : xs_rerank_kernel_u8<METRIC_IP>)
                                   : fmt == ROWS_I8  ? (l2 ? xs_rerank_kernel_i8<METRIC_L2> : xs_rerank_kernel_i8<METRIC_IP>)
                                   : fmt == ROWS_BF16 ? (l2 ? xs_rerank_kernel_bf16<METRIC_L2> : xs_rerank_kernel_bf16<METRIC_IP>)
                                   : fmt == ROWS_F8  ? (l2 ? xs_rerank_kernel_f8<METRIC_L2> : xs_rerank_kernel_f8<METRIC_IP>)
                                   : fmt == ROWS_F16 ? (l2 ? xs_rerank_kernel_f16<METRIC_L2> : xs_rerank_kernel_f16<METRIC_IP>)
                                                     : (l2 ? xs_rerank_kernel<METRIC_L2> : xs_rerank_kernel<METRIC_IP>);
  XsRerank ra{};
  ra.rows = rows; ra.labels = ix.labels; ra.queries = a.x.queries; ra.cand = static_cast<const unsigned char *>(a.cand);
  ra.qflag = a.qflag; ra.state = a.state; ra.fb_order = a.fb_order;
  ra.out_labels = a.x.out_labels; ra.out_dists = a.x.out_dists; ra.out_counts = a.x.out_counts;
  ra.dim = dim; ra.nq = nq; ra.k = k; ra.cap = xs_cap(k); ra.nruns = a.grid_x * 2;
  hipLaunchKernelGGL(rerank, dim3(nq), dim3(64), (size_t)dim * 4, stream, ra);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  // the flagged queries, by the scan: always enqueued, it finds its count on the device
  ExactArgs fb = a.x;
  fb.order = a.fb_order;
  return launch_exact_search_subset(ix, rows, fmt, fb, f, a.state, stream);
}

}  // namespace hs
