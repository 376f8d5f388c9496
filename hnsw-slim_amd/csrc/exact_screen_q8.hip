// exact_screen_q8.hip -- exact k-NN for byte queries over the byte rows of a resident index: exact_screen.hip's three
// steps with the screen on the integer matrix cores.  v_mfma_i32_32x32x32_i8 gives the exact integer dot product of 32 queries and 32
// rows over 32 positions, so the screened value is the exact integer distance; where the recipe's fp32 arithmetic is exact as well
// (exact_screen_margin.hpp, exact_screen_q8_interval) the interval fed to the lists is the point [r, r] and the screen keeps k rows
// plus ties.  Elsewhere it is 4r's margin around the rounded integer.  The lists, the re-rank (in the recipe's arithmetic, over the
// queries widened to fp32) and the fallback scan are exact_screen.hip's: no returned bit comes from a matrix instruction.
//
// xq_rownorms_kernel  per row, once per call: sum of squares and sum of the bytes as the MFMA sees them (u8: the value minus 128).
// xq_pack_kernel      per query, once per group: the bytes in the narrow copy's slot order (u8: sign bit flipped, i.e. minus 128 as
//                     i8), the fp32 copy, and XqQuery -- its share of the integer distance, its true norm, its inexact floor.
// xq_screen_kernel    a workgroup of 4 waves, a tile of 64 queries in LDS as bytes in operand layout [step][half][query][16]: one
//                     16-byte read is a lane's query operand of a step.  Wave (b, p) owns the 32 queries of half b and the 32-row
//                     units of parity p.  A step's row operand is one 16-byte global load straight from the narrow copy, loaded in
//                     groups of four steps, one group ahead; the first group of the wave's next unit is issued before the epilogue
//                     of this one, so row bytes are in flight under the hot loop.  No barrier in the row loop.
//                     Epilogue per accumulator element, in int32: V = xv_row + c p against the list's threshold less the query's
//                     share (one LDS word), AND the admission bit; a ballot that is almost always zero.  What passes goes through
//                     the exact interval, lo <= U and the ballot-serialised insert of exact_screen.hip.
//                     A tile longer than 512 bytes goes through LDS in slices of 256 between two barriers, each wave carrying two
//                     accumulator blocks across them (xs_screen_kernel<.., 4>'s scheme).
// Integer ranges at dim <= 4096: a sum of squares of values in [-128, 127] is <= 4096 * 2^14 = 2^26, of u8 values < 2^28.1; a sum
// of values has magnitude <= 2^19 (u8: < 2^20); |p| <= 2^26; D = qn' + xn' - 2 p <= 4 * 2^26 and |P| < 2^28.1: everything fits 32 bits.
#include <hip/hip_runtime.h>

#include <climits>

#include "bf_common.hpp"
#include "exact_screen_margin.hpp"
#include "exact_screen_q8_engine.hpp"
#include "narrow_rows.hpp"

namespace hs {

typedef int xq_i4v __attribute__((ext_vector_type(4)));
typedef int xq_i16v __attribute__((ext_vector_type(16)));

static constexpr uint32_t kXqWhole = 512;   // a tile up to this many positions is staged once
static constexpr uint32_t kXqSlice = 256;   // positions per slice of a longer one
static constexpr int kXqSliceUnits = 2;     // units a wave carries per slice (NU)

// the value the MFMA sees for a stored byte
template <bool U8> __device__ __forceinline__ int xq_seen(uint32_t byte) { return (int)(int8_t)(uint8_t)(U8 ? byte ^ 0x80u : byte); }

// ---- per row and per query integers -------------------------------------------------------------------------------------------
// 16 lanes per row, 16 rows per workgroup; the order of an integer sum does not matter, so the narrow row is read as it is stored.
template <bool U8>
__global__ void __launch_bounds__(256) xq_rownorms_kernel(const uint8_t *rows, uint32_t n, uint32_t dim, XqRow *out) {
  const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  uint32_t s2 = 0;
  int s1 = 0;
  if (r < n) {
    const uint32_t *x = reinterpret_cast<const uint32_t *>(rows + (size_t)r * dim);
    for (uint32_t i = l; i < (dim >> 2); i += 16) {
      const uint32_t w = x[i];
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int v = xq_seen<U8>((w >> (8 * b)) & 0xFFu);
        s2 += (uint32_t)(v * v);
        s1 += v;
      }
    }
  }
#pragma unroll
  for (int s = 8; s > 0; s >>= 1) {
    s2 += (uint32_t)__shfl_xor((int)s2, s, 16);
    s1 += __shfl_xor(s1, s, 16);
  }
  if (r < n && l == 0) out[r] = XqRow{s2, s1};
}

template <bool U8>
__global__ void __launch_bounds__(256) xq_widen_kernel(const uint8_t *src, size_t count, float *dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = U8 ? (float)src[i] : (float)(int8_t)src[i];
}

// One wave per query, four queries per workgroup.
template <int METRIC, bool U8>
__global__ void __launch_bounds__(256) xq_pack_kernel(const uint8_t *q, uint32_t nq, uint32_t dim, uint8_t *packed, float *wide, XqQuery *qinfo) {
  const uint32_t qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (qi >= nq) return;   // (a whole wave: no barrier below)
  const uint8_t *src = q + (size_t)qi * dim;
  uint32_t s2 = 0;
  int s1 = 0;
  for (uint32_t p = lane; p < dim; p += 64) {
    const uint32_t byte = src[narrow_elem(p, dim)];   // what slot p of a narrow row holds
    packed[(size_t)qi * dim + p] = (uint8_t)(U8 ? byte ^ 0x80u : byte);
    const int v = xq_seen<U8>(byte);
    s2 += (uint32_t)(v * v);
    s1 += v;
    const uint32_t nat = src[p];
    wide[(size_t)qi * dim + p] = U8 ? (float)nat : (float)(int8_t)nat;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    s2 += (uint32_t)__shfl_xor((int)s2, s);
    s1 += __shfl_xor(s1, s);
  }
  if (lane == 0) {
    // the true values are the seen ones plus 128 (u8): |q|^2 = s2 + 256 s1 + 16384 dim
    const uint32_t qn = U8 ? (uint32_t)((int)s2 + 256 * s1 + 16384 * (int)dim) : s2;
    const uint32_t xn_max = dim * (U8 ? 65025u : 16384u);
    XqQuery o;
    o.qa = METRIC == METRIC_L2 ? (int)s2 : (U8 ? -(128 * s1 + 16384 * (int)dim) : 0);
    o.qn = qn;
    o.floor_lo = exact_screen_q8_inexact_floor(METRIC == METRIC_IP, dim, qn, xn_max);
    o.pad = 0;
    qinfo[qi] = o;
  }
}

// ---- screen -------------------------------------------------------------------------------------------------------------------
struct XqScan {
  const uint8_t *rows;
  const uint8_t *deleted;
  const uint8_t *packed;
  const XqQuery *qinfo;
  const XqRow *rinfo;
  const uint32_t *order;
  unsigned char *cand;
  uint32_t *qflag;
  FilterArgs f;
  uint32_t n, dim, nq, k, cap, rows_per_block, slice;
};

// The integer pre-test of a list with bound U: a pair is kept when V = (L2: D, IP: -P) <= T.  It may only over-admit, since what
// passes still meets the exact lo <= U.  Pairs of the exact regime have lo = D resp. 1 - P as integers, so lo <= U is V <= floor(U)
// resp. V <= floor(U - 1) (the subtraction is exact in double).  Pairs of the inexact regime have lo >= floor_lo
// (exact_screen_q8_inexact_floor): while U < floor_lo none of them can pass lo <= U, and T = that floor loses nothing; once
// U >= floor_lo, or while the list holds fewer than k rows (U = +inf), T = INT_MAX admits everything to the exact test.
// Returned less the query's share qa of V, so that the hot loop compares the row's share alone.
__device__ __forceinline__ int xq_threshold(float U, float floor_lo, int qa, bool ip) {
  if (!(U < floor_lo)) return INT_MAX;
  double t = __builtin_floor((double)U - (ip ? 1.0 : 0.0));
  if (t >= 1073741824.0) return INT_MAX;
  if (t < -1073741824.0) t = -1073741824.0;   // (|V| < 2^29: nothing passes either way)
  return (int)t - qa;
}

struct XqGroup { xq_i4v v[4]; };
// steps [0, min(4, cnt)) of a row from x, which points at the lane's 16 bytes of the first
__device__ __forceinline__ void xq_load(XqGroup &g, const uint8_t *x, uint32_t cnt) {
#pragma unroll
  for (int i = 0; i < 4; i++)
    if ((uint32_t)i < cnt) g.v[i] = *reinterpret_cast<const xq_i4v *>(x + 32 * i);
}

// nsteps matrix steps of one unit against the queries at qA; cur holds the first group on entry and, on return, the first group of
// xnext (the wave's next unit; null: nothing), loaded under the last group's MFMAs and whatever the caller does next.
template <bool U8>
__device__ __forceinline__ void xq_steps(xq_i16v &acc, const uint8_t *x, uint32_t nsteps, const xq_i4v *qA, XqGroup &cur, const uint8_t *xnext, uint32_t nnext) {
  for (uint32_t t0 = 0; t0 < nsteps; t0 += 4) {
    XqGroup nxt = cur;
    if (t0 + 4 < nsteps) xq_load(nxt, x + 32 * (t0 + 4), nsteps - t0 - 4);
    else if (xnext) xq_load(nxt, xnext, nnext);
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (t0 + i < nsteps) {
        xq_i4v b = cur.v[i];
        if (U8) b ^= (int)0x80808080u;
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qA[(size_t)(t0 + i) * 2 * kXsTile], b, acc, 0, 0, 0);
      }
    cur = nxt;
  }
}

template <int METRIC, bool U8, int NU>
__device__ __forceinline__ void xq_screen_body(const XqScan &a, unsigned char *smem) {
  constexpr bool IP = METRIC == METRIC_IP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = wave & 1, p = wave >> 1, j = lane & 31, h = lane >> 5;
  const uint32_t dim = a.dim, k = a.k, cap = a.cap, slice = a.slice;
  uint8_t *qL = smem;                                                         // (slice / 32) x 2 x 64 x 16 bytes
  int *qa = reinterpret_cast<int *>(qL + (size_t)kXsTile * slice);            // 64
  uint32_t *qn = reinterpret_cast<uint32_t *>(qa + kXsTile);                  // 64
  float *qfloor = reinterpret_cast<float *>(qn + kXsTile);                    // 64
  uint32_t *slot_q = reinterpret_cast<uint32_t *>(qfloor + kXsTile);          // 64
  uint32_t *slot_f = slot_q + kXsTile;                                        // 64
  uint32_t *sizes = slot_f + kXsTile;                                         // 2 x 64
  float *ub = reinterpret_cast<float *>(sizes + 2 * kXsTile);                 // 2 x 64
  int *thr = reinterpret_cast<int *>(ub + 2 * kXsTile);                       // 2 x 64: xq_threshold of the list
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
    XqQuery qq{0, 0u, 0.f, 0u};
    if (qi != kXsNoSlot) qq = a.qinfo[qi];
    qa[tid] = qq.qa; qn[tid] = qq.qn; qfloor[tid] = qq.floor_lo;
    // a slot without a query or without a filter admits nothing: V <= INT_MIN never holds
    const int t = fi != kXsNoSlot ? INT_MAX : INT_MIN;
    thr[tid] = t; thr[kXsTile + tid] = t;
  }
  if (tid < (int)(2 * kXsTile)) { sizes[tid] = 0; ub[tid] = INFINITY; lflag[tid] = 0; }
  __syncthreads();
  // positions [p0, p0 + len) of the tile's packed queries into operand layout; 16 bytes per thread and turn
  auto stage = [&](uint32_t p0, uint32_t len) {
    for (uint32_t i = tid; i < kXsTile * (len >> 4); i += 256) {
      const uint32_t t = i & (kXsTile - 1), c = i >> 6, qi = slot_q[t];
      xq_i4v v = {0, 0, 0, 0};
      if (qi != kXsNoSlot) v = *reinterpret_cast<const xq_i4v *>(a.packed + (size_t)qi * dim + p0 + 16 * c);
      reinterpret_cast<xq_i4v *>(qL)[c * kXsTile + t] = v;
    }
  };
  if (NU == 1) {
    stage(0, dim);
    __syncthreads();
  }

  const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const uint32_t nsteps = dim >> 5;
  const xq_i4v *qA = reinterpret_cast<const xq_i4v *>(qL) + h * kXsTile + 32 * b + j;   // + 128 per step
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
  // the lane's 16 bytes of step 0 of row j of unit u (a row beyond n re-reads the chunk's first: it is never admitted)
  auto row_ptr = [&](uint32_t u) -> const uint8_t * {
    const uint32_t row = u * 32 + j;
    return a.rows + (size_t)(row < a.n ? row : r0) * dim + 16 * h;
  };
  // element v of lane (j, h): query slot 8 (v / 4) + 4 h + v % 4 of the half against row j of the unit
  auto epilogue = [&](uint32_t u, uint32_t w, uint32_t alive, const xq_i16v &acc) {
    const uint32_t base = u * 32, row = base + j;
    XqRow ri{0u, 0};
    if (row < a.n) ri = a.rinfo[row];
    const int xv = !IP ? (int)ri.norm : (U8 ? -128 * ri.sum : 0);
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const uint32_t tl = 8u * (v >> 2) + 4u * h + (v & 3), li = lbase + tl;
      const uint32_t awv = filt ? (uint32_t)__shfl((int)w, (int)tl) : alive;
      const int vr = !IP ? xv - 2 * acc[v] : xv - acc[v];
      const bool pass = ((awv >> j) & 1u) && vr <= thr[li];
      if (hs_ballot(pass) == 0) continue;
      // the exact test: the interval of the pair, lo <= U
      const int val = vr + qa[32 * b + tl];   // D, or -P
      const uint32_t xn = U8 ? (uint32_t)((int)ri.norm + 256 * ri.sum + 16384 * (int)dim) : ri.norm;
      float av;
      const float e = exact_screen_q8_interval(IP, dim, IP ? -val : val, qn[32 * b + tl], xn, &av);
      const float lo = av - e, hi = av + e;
      const bool fin = (lo - lo == 0.f) && (hi - hi == 0.f);
      if (pass && !fin) lflag[li] = 1;   // (several lanes may write the same 1)
      unsigned long long m = hs_ballot(pass && fin && lo <= ub[li]);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float hj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(hi), l));
        const float lj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lo), l));
        if (lane == 0) {
          const uint32_t sl = 8u * (v >> 2) + 4u * ((uint32_t)l >> 5) + (v & 3), lj_i = lbase + sl;
          xs_insert(lists + (size_t)lj_i * cap, sizes + lj_i, ub + lj_i, lflag + lj_i, k, cap, hj, lj, base + ((uint32_t)l & 31u));
          thr[lj_i] = xq_threshold(ub[lj_i], qfloor[32 * b + sl], qa[32 * b + sl], IP);
        }
        wave_sync();
      }
    }
  };

  if constexpr (NU == 1) {
    // the wave's units one after the other, the next one's admission and first rows fetched ahead; no barrier, so each wave runs
    // its own trip count
    uint32_t u = (r0 >> 5) + p, alive = 0, w = 0;
    bool act = false;
    XqGroup cur{};
    if (u * 32 < r1) {
      w = admit(u, alive);
      act = hs_ballot(w != 0) != 0;   // no query of this half may see a row of the unit: nothing of it is loaded
      if (act) xq_load(cur, row_ptr(u), nsteps);
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
        xq_i16v acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = 0;
        xq_steps<U8>(acc, row_ptr(u), nsteps, qA, cur, actn ? row_ptr(un) : nullptr, nsteps);
        epilogue(u, w, alive, acc);
      } else if (actn) {
        xq_load(cur, row_ptr(un), nsteps);
      }
      u = un; w = wn; alive = alive_n; act = actn;
    }
  } else {
    // (the trip count is the workgroup's: every wave meets the barriers)
    for (uint32_t ug = r0 >> 5; ug * 32 < r1; ug += 2 * NU) {
      uint32_t w[NU], alive[NU];
      bool act[NU];
      xq_i16v acc[NU];
#pragma unroll
      for (int i = 0; i < NU; i++) {
        const uint32_t u = ug + p + 2 * i;
        w[i] = 0; alive[i] = 0;
        if (u * 32 < r1) w[i] = admit(u, alive[i]);
        act[i] = hs_ballot(w[i] != 0) != 0;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[i][v] = 0;
      }
      for (uint32_t p0 = 0; p0 < dim; p0 += slice) {
        const uint32_t len = min(slice, dim - p0);
        __syncthreads();   // every wave is done with the slice before
        stage(p0, len);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NU; i++) {
          if (!act[i]) continue;
          const uint8_t *x = row_ptr(ug + p + 2 * i) + p0;
          XqGroup cur{};
          xq_load(cur, x, len >> 5);
          xq_steps<U8>(acc[i], x, len >> 5, qA, cur, nullptr, 0);
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
__global__ void __launch_bounds__(256) xq_screen_kernel_u8(const XqScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xq_screen_body<METRIC, true, NU>(a, smem);
}
template <int METRIC, int NU>
__global__ void __launch_bounds__(256) xq_screen_kernel_i8(const XqScan a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  xq_screen_body<METRIC, false, NU>(a, smem);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool xq_supported(int fmt, uint32_t dim, uint32_t k) {
  return (fmt == ROWS_U8 || fmt == ROWS_I8) && dim != 0 && (dim & 31u) == 0 && dim <= 4096 && k >= 1 && k <= 64;
}
uint32_t xq_slice(uint32_t dim) { return dim <= kXqWhole ? dim : kXqSlice; }
size_t xq_screen_lds_bytes(uint32_t dim, uint32_t k) {
  return (size_t)kXsTile * xq_slice(dim) + 5 * kXsTile * 4 + 4 * 2 * kXsTile * 4 + (size_t)2 * kXsTile * xs_cap(k) * sizeof(XsCand);
}
const char *xq_kernel_name(int fmt) { return fmt == ROWS_U8 ? "hs::xq_screen_kernel_u8" : "hs::xq_screen_kernel_i8"; }

hipError_t launch_exact_q8_rownorms(const DevIndex &ix, const void *rows, int fmt, XqRow *rinfo, hipStream_t stream) {
  if (!ix.n) return hipSuccess;
  if (!rows || (fmt != ROWS_U8 && fmt != ROWS_I8) || (ix.dim & 3u)) return hipErrorInvalidValue;
  const dim3 g((ix.n + 15) / 16);
  if (fmt == ROWS_U8) hipLaunchKernelGGL(xq_rownorms_kernel<true>, g, dim3(256), 0, stream, static_cast<const uint8_t *>(rows), ix.n, ix.dim, rinfo);
  else hipLaunchKernelGGL(xq_rownorms_kernel<false>, g, dim3(256), 0, stream, static_cast<const uint8_t *>(rows), ix.n, ix.dim, rinfo);
  return hipGetLastError();
}

hipError_t launch_exact_q8_widen(const void *src, int fmt, size_t count, float *dst, hipStream_t stream) {
  if (!count) return hipSuccess;
  if (fmt != ROWS_U8 && fmt != ROWS_I8) return hipErrorInvalidValue;
  const dim3 g((unsigned)((count + 255) / 256));
  if (fmt == ROWS_U8) hipLaunchKernelGGL(xq_widen_kernel<true>, g, dim3(256), 0, stream, static_cast<const uint8_t *>(src), count, dst);
  else hipLaunchKernelGGL(xq_widen_kernel<false>, g, dim3(256), 0, stream, static_cast<const uint8_t *>(src), count, dst);
  return hipGetLastError();
}

hipError_t launch_exact_screen_q8(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const XqArgs &q, const FilterArgs *f, hipStream_t stream) {
  const uint32_t dim = ix.dim, nq = a.x.nq, k = a.x.k;
  if (!xq_supported(fmt, dim, k) || nq == 0 || a.x.queries != q.wide) return hipErrorInvalidValue;
  if (!rows && ix.n) return hipErrorInvalidDevicePointer;
  const bool l2 = ix.metric == METRIC_L2, u8 = fmt == ROWS_U8;
  hipError_t e;
  if ((e = launch_exact_screen_init(a, stream)) != hipSuccess) return e;
  void (*pack)(const uint8_t *, uint32_t, uint32_t, uint8_t *, float *, XqQuery *) =
      u8 ? (l2 ? xq_pack_kernel<METRIC_L2, true> : xq_pack_kernel<METRIC_IP, true>) : (l2 ? xq_pack_kernel<METRIC_L2, false> : xq_pack_kernel<METRIC_IP, false>);
  hipLaunchKernelGGL(pack, dim3((nq + 3) / 4), dim3(256), 0, stream, static_cast<const uint8_t *>(q.queries), nq, dim, q.packed, q.wide, q.qinfo);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  const uint32_t slice = xq_slice(dim);
  void (*screen)(const XqScan);
#define HS_XQ_PICK(NU) \
  screen = u8 ? (l2 ? xq_screen_kernel_u8<METRIC_L2, NU> : xq_screen_kernel_u8<METRIC_IP, NU>) : (l2 ? xq_screen_kernel_i8<METRIC_L2, NU> : xq_screen_kernel_i8<METRIC_IP, NU>)
  if (slice >= dim) HS_XQ_PICK(1);
  else HS_XQ_PICK(kXqSliceUnits);
#undef HS_XQ_PICK
  const size_t lds = xq_screen_lds_bytes(dim, k);
  if (lds > 48 * 1024) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(screen), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  XqScan sa{};
  sa.rows = static_cast<const uint8_t *>(rows); sa.deleted = ix.has_deleted ? ix.deleted : nullptr;
  sa.packed = q.packed; sa.qinfo = q.qinfo; sa.rinfo = q.rinfo; sa.order = a.x.order;
  sa.cand = static_cast<unsigned char *>(a.cand); sa.qflag = a.qflag;
  if (f) sa.f = *f;
  sa.n = ix.n; sa.dim = dim; sa.nq = nq; sa.k = k; sa.cap = xs_cap(k); sa.rows_per_block = a.rows_per_block; sa.slice = slice;
  hipLaunchKernelGGL(screen, dim3(a.grid_x, (nq + kXsTile - 1) / kXsTile), dim3(256), lds, stream, sa);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_exact_screen_finish(ix, rows, fmt, a, f, stream);
}

}  // namespace hs
