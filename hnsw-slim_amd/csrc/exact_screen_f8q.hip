// exact_screen_f8q.hip -- exact k-NN for fp8 (OCP E4M3) queries over the fp8 rows of a resident index: exact_screen.hip's
// three steps with the screen on the fp8 matrix cores.  v_mfma_f32_32x32x64_f8f6f4 multiplies 32 queries and 32 rows over 64 positions;
// a product of two E4M3 values has an 8-bit significand and lies in [2^-18, 448^2], so it is exact in fp32 and only the accumulation
// rounds.  The screened value a and its margin e (exact_screen_margin.hpp, exact_screen_f8_margin) feed the lists of exact_screen.hip;
// the lists' insertion (xs_insert), the re-rank in the recipe's arithmetic over the queries widened to fp32 and the fallback scan
// (launch_exact_screen_finish) are that file's: no returned bit comes from a matrix instruction.
//
// xf_rowinfo_kernel  per row, once per call: |x|^2 summed exactly as xs_norms_kernel<hs_f8> sums it, and the count of the row's
//                    subnormal bytes (nonzero, below 2^-6).
// xf_pack_kernel     per query, once per group, one wave: the bytes in the narrow copy's slot order, the fp32 copy in natural order,
//                    and XhInfo -- the norm over the slot order in xs_norms_kernel's summation, the count of subnormal bytes.
// xf_screen_kernel   a workgroup of 4 waves, a tile of 64 queries in LDS as bytes.  Wave (b, p) owns the 32 queries of half b and the
//                    32-row units of parity p, as in the fp16 screen.  A matrix step covers 64 slots; lane (j, h) of it holds 32 bytes
//                    of each operand, slots [64 t + 32 h, +32):
//                      rows     straight from the narrow copy, two 16-byte global loads at row j's byte 64 t + 32 h (a row is dim
//                               bytes, 16-byte aligned); the k index of a product may be permuted as long as both operands agree, so
//                               slot order is used as it lies;
//                      queries  LDS layout [step][16-byte half c][h][query][16]: the lane's operand is two 16-byte reads, and in each
//                               the 32 lanes of a group read 512 contiguous bytes -- no bank is asked twice in a quarter wave.
//                    Row loads go in groups of two steps (128 slots, 16 VGPRs), one group ahead of the MFMAs; the first group of the
//                    wave's next unit is issued before the epilogue of this one.  No barrier in the row loop.
//                    dim % 64 != 0 (16, 48, 80, ...) ends in a step whose missing 16-byte halves are zero bytes in both operands --
//                    not loaded, and staged as zeros; byte 0 is +0.0, so they add nothing.
//                    Epilogue per accumulator element: the fp16 screen's pre-test (exact_screen_margin.hpp, "the pre-test": one FMA,
//                    one compare, it can only over-admit), then for what passes a, e, lo, hi as exact_screen.hip forms them, lo <= U,
//                    and through a ballot into the list by lane 0, which refreshes the bound.  A row or a query with subnormal bytes,
//                    a query whose norm is not finite (a NaN byte) and a list below k rows send every pair to the full test.
//                    A tile longer than 256 positions goes through LDS in slices of 256 (four steps, 16 KiB) between two barriers,
//                    each wave carrying two accumulator blocks across them, as the fp16 screen does.
#include <hip/hip_runtime.h>

#include "bf_common.hpp"
#include "exact_screen_f8q_engine.hpp"
#include "exact_screen_margin.hpp"
#include "narrow_rows.hpp"

namespace hs {

typedef int xf_i8v __attribute__((ext_vector_type(8)));
typedef float xf_f16v __attribute__((ext_vector_type(16)));

static constexpr uint32_t kXfWhole = 256;   // a tile up to this many positions (16 KiB) is staged once, where it fits beside the lists
static constexpr uint32_t kXfSlice = 256;   // positions per slice of a longer one: 4 matrix steps
static constexpr int kXfSliceUnits = 2;     // units a wave carries per slice (NU)
static constexpr int kXfGroup = 2;          // matrix steps per group of row loads (128 slots, 16 VGPRs, and as many for the group ahead)
static constexpr int kXfSliceGroup = 1;     // ... in the sliced kernel, whose two accumulator blocks leave room for less

// a nonzero byte of magnitude below 2^-6: exponent field 0
__device__ __forceinline__ uint32_t xf_is_sub(uint8_t b) {
  const uint32_t m = b & 0x7Fu;
  return m != 0u && m < 8u;
}
__device__ __forceinline__ float xf_wide(uint8_t b) { return (float)hs_f8{b}; }   // (the decode on the bits: what xs_norms_kernel<hs_f8> sums)

// ---- per row and per query ----------------------------------------------------------------------------------------------------
// 16 lanes per row, 16 rows per workgroup; the row is summed in the order it is stored -- xs_norms_kernel's loop, fma and reduction.
__global__ void __launch_bounds__(256) xf_rowinfo_kernel(const uint8_t *rows, uint32_t n, uint32_t dim, XhInfo *out) {
  const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  float s = 0.f;
  uint32_t c = 0;
  if (r < n) {
    const uint8_t *x = rows + (size_t)r * dim;
    for (uint32_t i = l; i < dim; i += 16) {
      const uint8_t b = x[i];
      const float e = xf_wide(b);
      s = __builtin_fmaf(e, e, s);
      c += xf_is_sub(b);
    }
  }
#pragma unroll
  for (int w = 8; w > 0; w >>= 1) {
    s += __shfl_xor(s, w, 16);
    c += (uint32_t)__shfl_xor((int)c, w, 16);
  }
  if (r < n && l == 0) out[r] = XhInfo{s, c};
}

__global__ void __launch_bounds__(256) xf_widen_kernel(const uint8_t *src, size_t count, float *dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = xf_wide(src[i]);
}

// One wave per query, four queries per workgroup.
__global__ void __launch_bounds__(256) xf_pack_kernel(const uint8_t *q, uint32_t nq, uint32_t dim, uint8_t *packed, float *wide, XhInfo *qinfo) {
  const uint32_t qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (qi >= nq) return;   // (a whole wave: no barrier below)
  const uint8_t *src = q + (size_t)qi * dim;
  uint32_t c = 0;
  for (uint32_t p = lane; p < dim; p += 64) {
    const uint8_t b = src[narrow_elem(p, dim)];   // what slot p of a narrow row holds
    packed[(size_t)qi * dim + p] = b;
    c += xf_is_sub(b);
    wide[(size_t)qi * dim + p] = xf_wide(src[p]);
  }
  // the norm over the slot order, 16 lanes as xs_norms_kernel (each quarter of the wave forms the same sum)
  float s = 0.f;
  for (uint32_t i = lane & 15u; i < dim; i += 16) {
    const float e = xf_wide(src[narrow_elem(i, dim)]);
    s = __builtin_fmaf(e, e, s);
  }
#pragma unroll
  for (int w = 8; w > 0; w >>= 1) s += __shfl_xor(s, w, 16);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) c += (uint32_t)__shfl_xor((int)c, w);
  if (lane == 0) qinfo[qi] = XhInfo{s, c};
}

// ---- screen -------------------------------------------------------------------------------------------------------------------
struct XfScan {
  const unsigned char *rows;
  const uint8_t *deleted;
  const unsigned char *packed;
  const XhInfo *qinfo, *rinfo;
  const uint32_t *order;
  unsigned char *cand;
  uint32_t *qflag;
  FilterArgs f;
  uint32_t n, dim, nq, k, cap, rows_per_block, slice;
};

// the bytes of the LDS tile for `len` positions: whole steps, [step][c][h][64 queries][16]
__host__ __device__ inline uint32_t xf_tile_bytes(uint32_t len) { return (len + 63u) / 64u * 64u * kXsTile; }

template <int G> struct XfGroup { uint4 v[G][2]; };
__device__ __forceinline__ xf_i8v xf_operand(const uint4 lo, const uint4 hi) {
  return xf_i8v{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}
// Steps [t0, t0 + G) below nsteps of a row.  x points at the lane's byte 32 h of the row's first position; lim is the number
// of bytes from there to the end of the positions in play (may be <= 0 for h = 1): a 16-byte half at or beyond it is zero, not read.
template <int G>
__device__ __forceinline__ void xf_load(XfGroup<G> &g, const unsigned char *x, uint32_t t0, uint32_t nsteps, int lim) {
#pragma unroll
  for (int i = 0; i < G; i++)
    if (t0 + i < nsteps) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        const int off = 64 * (int)(t0 + i) + 16 * c;
        g.v[i][c] = off < lim ? *reinterpret_cast<const uint4 *>(x + off) : make_uint4(0u, 0u, 0u, 0u);
      }
    }
}

// nsteps matrix steps of one unit against the queries at qA; cur holds the first group on entry and, on return, the first group of
// xnext (the wave's next unit; null: nothing), loaded under the last group's MFMAs and whatever the caller does next.
template <int G>
__device__ __forceinline__ void xf_steps(xf_f16v &acc, const unsigned char *x, uint32_t nsteps, int lim, const uint4 *qA, XfGroup<G> &cur, const unsigned char *xnext) {
  for (uint32_t t0 = 0; t0 < nsteps; t0 += G) {
    XfGroup<G> nxt = cur;
    if (t0 + G < nsteps) xf_load(nxt, x, t0 + G, nsteps, lim);
    else if (xnext) xf_load(nxt, xnext, 0, nsteps, lim);
#pragma unroll
    for (int i = 0; i < G; i++)
      if (t0 + i < nsteps) {
        const uint4 *qs = qA + (size_t)(t0 + i) * 4 * kXsTile;
        // both format selectors 0: fp8 E4M3; zero scale operands select the unscaled instruction
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xf_operand(qs[0], qs[2 * kXsTile]), xf_operand(cur.v[i][0], cur.v[i][1]), acc, 0, 0, 0, 0, 0, 0);
      }
    cur = nxt;
  }
}

template <int METRIC, int NU>
__device__ __forceinline__ void xf_screen_body(const XfScan &a, unsigned char *smem) {
  constexpr bool IP = METRIC == METRIC_IP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = wave & 1, p = wave >> 1, j = lane & 31, h = lane >> 5;
  const uint32_t dim = a.dim, k = a.k, cap = a.cap, slice = a.slice, rowbytes = a.dim;
  unsigned char *qL = smem;                                                   // xf_tile_bytes(slice)
  float *qn = reinterpret_cast<float *>(qL + xf_tile_bytes(slice));           // 64
  uint32_t *qsub = reinterpret_cast<uint32_t *>(qn + kXsTile);                // 64
  float *qsh = reinterpret_cast<float *>(qsub + kXsTile);                     // 64: exact_screen_f16_pre_query
  uint32_t *slot_q = reinterpret_cast<uint32_t *>(qsh + kXsTile);             // 64
  uint32_t *slot_f = slot_q + kXsTile;                                        // 64
  uint32_t *sizes = slot_f + kXsTile;                                         // 2 x 64
  float *ub = reinterpret_cast<float *>(sizes + 2 * kXsTile);                 // 2 x 64
  float *thr = ub + 2 * kXsTile;                                              // 2 x 64: exact_screen_f16_pre_bound of the list
  uint32_t *lflag = reinterpret_cast<uint32_t *>(thr + 2 * kXsTile);          // 2 x 64
  XsCand *lists = reinterpret_cast<XsCand *>(lflag + 2 * kXsTile);            // 2 x 64 x cap
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
    XhInfo qq{0.f, 0u};
    if (qi != kXsNoSlot) qq = a.qinfo[qi];
    qn[tid] = qq.norm; qsub[tid] = qq.sub;
    qsh[tid] = exact_screen_f16_pre_query(IP, dim, qq.norm);
    // a list below k rows sends every pair to the full test; a slot without a query or without a filter passes no pre-test (its
    // products are zeros, so the pre-test's value is finite) and is stopped at the full test where a row skips the pre-test
    const float t = fi != kXsNoSlot ? INFINITY : -INFINITY;
    thr[tid] = t; thr[kXsTile + tid] = t;
  }
  if (tid < (int)(2 * kXsTile)) { sizes[tid] = 0; ub[tid] = INFINITY; lflag[tid] = 0; }
  __syncthreads();
  // positions [p0, p0 + len) of the tile's packed queries into operand layout, 16 bytes per thread and turn; the 16-byte halves of the
  // last step beyond len are zeros
  auto stage = [&](uint32_t p0, uint32_t len) {
    const uint32_t chunks = (len + 63u) / 64u * 4u;
    for (uint32_t i = tid; i < kXsTile * chunks; i += 256) {
      const uint32_t t = i & (kXsTile - 1), ch = i >> 6, qi = slot_q[t];
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (qi != kXsNoSlot && 16u * ch < len) v = *reinterpret_cast<const uint4 *>(a.packed + (size_t)qi * rowbytes + p0 + 16 * ch);
      const uint32_t st = ch >> 2, hh = (ch >> 1) & 1u, c = ch & 1u;
      reinterpret_cast<uint4 *>(qL)[((st * 2 + c) * 2 + hh) * kXsTile + t] = v;
    }
  };
  if (NU == 1) {
    stage(0, dim);
    __syncthreads();
  }

  const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const uint32_t nsteps = (dim + 63u) >> 6;
  const uint4 *qA = reinterpret_cast<const uint4 *>(qL) + h * kXsTile + 32 * b + j;   // + 256 per step, + 128 for the second half
  const uint32_t lbase = p * kXsTile + 32 * b;   // this wave's lists: lbase + local slot
  const bool filt = a.f.rows != nullptr;

  // Admission of unit u (u * 32 < r1), as exact_search.hip's exact_admit: `alive` the rows below n without a delete mark (uniform), w
  // the word of local slot `lane` (lanes 0 .. 31).
  auto admit = [&](uint32_t u, uint32_t &alive) -> uint32_t {
    const uint32_t base = u * 32, left = a.n - base;
    alive = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
    if (a.deleted) {
      const uint32_t idx = base + j;
      const bool del = lane < 32 && idx < a.n && a.deleted[idx] != 0;
      alive &= ~(uint32_t)hs_ballot(del);
    }
    uint32_t w = 0;
    if (lane < 32) {
      const uint32_t fi = slot_f[32 * b + lane];
      if (fi != kXsNoSlot) w = filt ? a.f.rows[(size_t)fi * a.f.stride + u] : 0xFFFFFFFFu;
    }
    return w & alive;
  };
  // the lane's byte 32 h of row j of unit u (a row beyond n re-reads the chunk's first: it is never admitted)
  auto row_ptr = [&](uint32_t u) -> const unsigned char * {
    const uint32_t row = u * 32 + j;
    return a.rows + (size_t)(row < a.n ? row : r0) * rowbytes + 32 * h;
  };
  // element v of lane (j, h): query slot 8 (v / 4) + 4 h + v % 4 of the half against row j of the unit
  auto epilogue = [&](uint32_t u, uint32_t w, uint32_t alive, const xf_f16v &acc) {
    const uint32_t base = u * 32, row = base + j;
    XhInfo ri{0.f, 0u};
    if (row < a.n) ri = a.rinfo[row];
    const float xrow = exact_screen_f16_pre_row(IP, dim, ri.norm);
    const bool full = ri.sub != 0u;   // (a row's norm is finite: its bytes are)
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const uint32_t tl = 8u * (v >> 2) + 4u * h + (v & 3), li = lbase + tl;
      const uint32_t awv = filt ? (uint32_t)__shfl((int)w, (int)tl) : alive;
      const float dot = acc[v];
      const float pre = IP ? __builtin_fmaf(qsh[32 * b + tl], xrow, -dot) : __builtin_fmaf(-2.f, dot, xrow);
      const bool pass = ((awv >> j) & 1u) && (full || !(pre > thr[li]));
      if (hs_ballot(pass) == 0) continue;
      // the full test: the interval of the pair, lo <= U
      const float qq = qn[32 * b + tl];
      const float av = !IP ? (qq + ri.norm) - 2.f * dot : 1.f - dot;
      const float e = exact_screen_f8_margin(IP, dim, qq, ri.norm, qsub[32 * b + tl], ri.sub);
      const float lo = av - e, hi = av + e;
      const bool fin = (lo - lo == 0.f) && (hi - hi == 0.f);
      const bool adm = pass && slot_f[32 * b + tl] != kXsNoSlot;
      if (adm && !fin) lflag[li] = 1;   // (several lanes may write the same 1)
      unsigned long long m = hs_ballot(adm && fin && lo <= ub[li]);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float hj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(hi), l));
        const float lj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lo), l));
        if (lane == 0) {
          const uint32_t sl = 8u * (v >> 2) + 4u * ((uint32_t)l >> 5) + (v & 3), lj_i = lbase + sl, s = 32 * b + sl;
          xs_insert(lists + (size_t)lj_i * cap, sizes + lj_i, ub + lj_i, lflag + lj_i, k, cap, hj, lj, base + ((uint32_t)l & 31u));
          const float qs = qn[s];
          const bool qfull = qsub[s] != 0u || !(qs - qs == 0.f);
          thr[lj_i] = qfull ? INFINITY : exact_screen_f16_pre_bound(IP, dim, ub[lj_i], qsh[s]);
        }
        wave_sync();
      }
    }
  };

  if constexpr (NU == 1) {
    // the wave's units one after the other, the next one's admission and first rows fetched ahead; no barrier, so each wave runs
    // its own trip count
    const int lim = (int)dim - 32 * (int)h;
    uint32_t u = (r0 >> 5) + p, alive = 0, w = 0;
    bool act = false;
    XfGroup<kXfGroup> cur{};
    if (u * 32 < r1) {
      w = admit(u, alive);
      act = hs_ballot(w != 0) != 0;   // no query of this half may see a row of the unit: nothing of it is loaded
      if (act) xf_load(cur, row_ptr(u), 0, nsteps, lim);
    }
    while (u * 32 < r1) {
      const uint32_t un = u + 2;
      uint32_t alive_n = 0, wn = 0;
      bool actn = false;
      if (un * 32 < r1) {
        wn = admit(un, alive_n);
        actn = hs_ballot(wn != 0) != 0;
      }
      if (act) {
        xf_f16v acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = 0.f;
        xf_steps(acc, row_ptr(u), nsteps, lim, qA, cur, actn ? row_ptr(un) : nullptr);
        epilogue(u, w, alive, acc);
      } else if (actn) {
        xf_load(cur, row_ptr(un), 0, nsteps, lim);
      }
      u = un; w = wn; alive = alive_n; act = actn;
    }
  } else {
    // (the trip count is the workgroup's: every wave meets the barriers)
    for (uint32_t ug = r0 >> 5; ug * 32 < r1; ug += 2 * NU) {
      uint32_t w[NU], alive[NU];
      bool act[NU];
      xf_f16v acc[NU];
#pragma unroll
      for (int i = 0; i < NU; i++) {
        const uint32_t u = ug + p + 2 * i;
        w[i] = 0; alive[i] = 0;
        if (u * 32 < r1) w[i] = admit(u, alive[i]);
        act[i] = hs_ballot(w[i] != 0) != 0;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[i][v] = 0.f;
      }
      for (uint32_t p0 = 0; p0 < dim; p0 += slice) {
        const uint32_t len = min(slice, dim - p0), ns = (len + 63u) >> 6;
        const int lim = (int)len - 32 * (int)h;
        __syncthreads();   // every wave is done with the slice before
        stage(p0, len);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NU; i++) {
          if (!act[i]) continue;
          const unsigned char *x = row_ptr(ug + p + 2 * i) + p0;
          XfGroup<kXfSliceGroup> cur{};
          xf_load(cur, x, 0, ns, lim);
          xf_steps(acc[i], x, ns, lim, qA, cur, nullptr);
        }
      }
#pragma unroll
      for (int i = 0; i < NU; i++)
        if (act[i]) epilogue(ug + p + 2 * i, w[i], alive[i], acc[i]);
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
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) xf_screen_kernel(const XfScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xf_screen_body<METRIC, NU>(a, smem);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool xf_supported(int fmt, uint32_t dim, uint32_t k) { return fmt == ROWS_F8 && dim != 0 && (dim & 15u) == 0 && dim <= 4096 && k >= 1 && k <= 64; }
static size_t xf_lds_for(uint32_t slice, uint32_t k) {
  return (size_t)xf_tile_bytes(slice) + 5 * kXsTile * 4 + 4 * 2 * kXsTile * 4 + (size_t)2 * kXsTile * xs_cap(k) * sizeof(XsCand);
}
uint32_t xf_slice(uint32_t dim, uint32_t k) { return dim <= kXfWhole && xf_lds_for(dim, k) <= 160 * 1024 ? dim : kXfSlice; }
size_t xf_screen_lds_bytes(uint32_t dim, uint32_t k) { return xf_lds_for(xf_slice(dim, k), k); }
const char *xf_kernel_name() { return "hs::xf_screen_kernel"; }

hipError_t launch_exact_f8q_rowinfo(const DevIndex &ix, const void *rows, XhInfo *rinfo, hipStream_t stream) {
  if (!ix.n) return hipSuccess;
  if (!rows) return hipErrorInvalidDevicePointer;
  hipLaunchKernelGGL(xf_rowinfo_kernel, dim3((ix.n + 15) / 16), dim3(256), 0, stream, static_cast<const uint8_t *>(rows), ix.n, ix.dim, rinfo);
  return hipGetLastError();
}

hipError_t launch_exact_f8q_widen(const void *src, size_t count, float *dst, hipStream_t stream) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(xf_widen_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, static_cast<const uint8_t *>(src), count, dst);
  return hipGetLastError();
}

hipError_t launch_exact_screen_f8q(const DevIndex &ix, const void *rows, const ScreenArgs &a, const XhArgs &q, const FilterArgs *f, hipStream_t stream) {
  const uint32_t dim = ix.dim, nq = a.x.nq, k = a.x.k;
  if (!xf_supported(ROWS_F8, dim, k) || nq == 0 || a.x.queries != q.wide) return hipErrorInvalidValue;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2;
  hipError_t e;
  if ((e = launch_exact_screen_init(a, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(xf_pack_kernel, dim3((nq + 3) / 4), dim3(256), 0, stream, static_cast<const uint8_t *>(q.queries), nq, dim,
                     reinterpret_cast<uint8_t *>(q.packed), q.wide, q.qinfo);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  const uint32_t slice = xf_slice(dim, k);
  void (*screen)(const XfScan) = slice >= dim ? (l2 ? xf_screen_kernel<METRIC_L2, 1> : xf_screen_kernel<METRIC_IP, 1>)
                                              : (l2 ? xf_screen_kernel<METRIC_L2, kXfSliceUnits> : xf_screen_kernel<METRIC_IP, kXfSliceUnits>);
  const size_t lds = xf_screen_lds_bytes(dim, k);
  if (lds > 48 * 1024) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(screen), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  XfScan sa{};
  sa.rows = static_cast<const unsigned char *>(rows); sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.packed = reinterpret_cast<const unsigned char *>(q.packed); sa.qinfo = q.qinfo; sa.rinfo = q.rinfo; sa.order = a.x.order;
  sa.cand = static_cast<unsigned char *>(a.cand); sa.qflag = a.qflag;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = dim; sa.nq = nq; sa.k = k; sa.cap = xs_cap(k); sa.rows_per_block = a.rows_per_block; sa.slice = slice;
  hipLaunchKernelGGL(screen, dim3(a.grid_x, (nq + kXsTile - 1) / kXsTile), dim3(256), lds, stream, sa);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_exact_screen_finish(ix, rows, ROWS_F8, a, f, stream);
}

}  // namespace hs
