// exact_screen_margin.hpp -- the proven bound between the screened distance of exact_screen.hip and the project's fp32 recipe
// (dist_recipe.hpp).  One source for the kernel and for the host (hs_debug_exact_screen_margin); derivation: DESIGN.md 4r.
//
// r = the recipe's distance of (q, x); a = the screened value from fp32 norms qn2 = fl(|q|^2), xn2 = fl(|x|^2) and an fp32 dot product
// accumulated in ANY order (fused or not):  L2  a = fl(fl(qn2 + xn2) - 2 p),  IP  a = fl(1 - p).  With u = 2^-24 and d = dim <= 4096:
//   L2  |a - r| <= (4 d + 7) u S (1 + o(1)),  S = |q|^2 + |x|^2      -> e = 8 (d + 8) u fl(qn2 + xn2)
//   IP  |a - r| <= (2 d + 2) u (P + 1) (1 + o(1)),  P = |q| |x|      -> e = 4 (d + 8) u (fl(sqrt qn2) fl(sqrt xn2) + 1)
// The factor of about two left over pays for the norms being fp32 results themselves, the roundings of e, lo = a - e and hi = a + e, and
// the 1 / (1 - d u) of the gamma bounds.  The term (d + 8) 2^-120 covers products and inputs lost to underflow or flushed to zero.
// +inf -- "cannot decide", the query falls back to the scan -- when a norm is not finite or so large that the recipe may overflow
// where the screen does not (S or P above 2^125).
// Sign does not enter: the rounding bounds are stated on sum |q_i| |x_i| <= |q| |x| <= S / 2 and on the squares, the premises on the
// norms and dim alone, so the bound serves rows with negative values (fp32, fp16 and i8 rows) as it serves u8 rows.
#pragma once
#include "hd.hpp"

namespace hs {

HS_HD float exact_screen_margin(int metric_ip, uint32_t dim, float qn2, float xn2) {
  const float kBig = 4.2535296e37f;                   // 2^125
  const float c = (float)(dim + 8u) * 5.9604645e-8f;  // (d + 8) 2^-24, exact for d <= 4096
  const float tiny = (float)(dim + 8u) * 7.5231638e-37f;   // (d + 8) 2^-120
  if (!(qn2 >= 0.f) || !(xn2 >= 0.f)) return __builtin_inff();   // NaN
  if (metric_ip) {
    const float p = __builtin_sqrtf(qn2) * __builtin_sqrtf(xn2);
    if (!(p <= kBig)) return __builtin_inff();
    return 4.f * c * (p + 1.f) + tiny;
  }
  const float s = qn2 + xn2;
  if (!(s <= kBig)) return __builtin_inff();
  return 8.f * c * s + tiny;
}

// The integer screen of exact_screen_q8.hip: rows and queries are bytes, v is the exact integer L2 distance D or inner
// product P (int32 at dim <= 4096), qn / xn the exact integer squared norms of the true values.  Returns e and writes a with
// |a - r| <= e for the recipe's r:
//   L2, D < 2^24         a = (float)D exactly, e = 0: every partial sum of the recipe is a sum of squares of integers, an integer
//                        <= D, so each fp32 operation is exact in any order, fused or not, and r = D.
//   IP, qn xn < 2^48     a = 1 - (float)P exactly, e = 0: every partial sum is an integer bounded by sum |q_i x_i| <= |q| |x| < 2^24,
//                        so the sum is P exactly, and 1 - P, an integer of magnitude <= 2^24, is exact as well.
//   otherwise            a = fl(D) or fl(1 - fl(P)), e = exact_screen_margin over (float)qn, (float)xn.  That margin bounds
//                        |a' - r| for an fp32 screen a' by E_recipe + E_screen', E_recipe <= (2 d + 4) u S (L2), (d + 2) u (P' + 1) (IP,
//                        P' = |q| |x|) the recipe's own rounding and E_screen' of the same size.  The integer screen's error is one or two
//                        roundings:  L2  |fl(D) - D| <= u D <= 2 u S;  IP  |a - (1 - P)| <= u |P| + u |1 - fl(P)| <= 2 u (P' + 1) (1 + u).
//                        So |a - r| <= E_recipe + 2 u S <= (2 d + 6) u S < (4 d + 7) u S, and (d + 4) u (P' + 1) <= (2 d + 2) u (P' + 1)
//                        for d >= 2; the norms, one rounding off their integers, sit inside the factor of two the margin keeps.
HS_HD float exact_screen_q8_interval(int metric_ip, uint32_t dim, int32_t v, uint32_t qn, uint32_t xn, float *a) {
  if (metric_ip) {
    *a = 1.f - (float)v;
    if ((uint64_t)qn * (uint64_t)xn < (1ull << 48)) return 0.f;
  } else {
    *a = (float)v;
    if (v < (1 << 24)) return 0.f;
  }
  return exact_screen_margin(metric_ip, dim, (float)qn, (float)xn);
}

// The smallest lo = fl(a - e) any pair of the inexact regime can have for a query of squared norm qn against rows of squared norm
// <= xn_max; +inf when no pair of the query can be inexact.  Every operation involved is monotone, so evaluating at the extreme
// arguments bounds every pair:  L2  a >= 2^24 and e <= e(xn_max);  IP  fl(P) <= pmax, a float >= |q| sqrt(xn_max), and e <= e(xn_max).
// Below this value the screen's integer pre-test alone decides (exact_screen_q8.hip, xq_threshold).
HS_HD float exact_screen_q8_inexact_floor(int metric_ip, uint32_t dim, uint32_t qn, uint32_t xn_max) {
  const float e = exact_screen_margin(metric_ip, dim, (float)qn, (float)xn_max);
  if (metric_ip) {
    if ((uint64_t)qn * (uint64_t)xn_max < (1ull << 48)) return __builtin_inff();
    const float pmax = (float)(__builtin_sqrt((double)qn * (double)xn_max) * 1.000001 + 1.0);
    return (1.f - pmax) - e;
  }
  if (2ull * ((uint64_t)qn + (uint64_t)xn_max) < (1ull << 24)) return __builtin_inff();   // D <= 2 (|q|^2 + |x|^2)
  return 16777216.f - e;
}

// The half-precision screen of exact_screen_f16q.hip: rows and queries are IEEE halves, the dot product p comes from
// v_mfma_f32_32x32x16_f16, the norms qn2, xn2 from fp32 sums of the widened values, a is formed as above.  A product of two halves is
// exact in fp32 (11 x 11 significand bits, exponents in [-48, 32]), so all of the screen's error is in additions.  Nothing is assumed
// of the matrix pipeline but that each of its additions errs by at most one ulp (2 u relative), in any order:
//   L2  recipe |r - D| <= 2 gamma_(d+2) S;  screen: the norms (d - 1) u S (exact squares) plus one rounding of their sum, the dot
//       |p - q.x| <= 2 d u sum |q_i x_i| <= d u S and doubled exactly, the last subtraction <= 2 u S:  |a - r| <= (5 d + 8) u S.
//   IP  recipe (d + 2) u (P + 1);  screen 2 d u P + u |1 - p|:  |a - r| <= (3 d + 3) u (P + 1).
// So 4r's two expressions stand, with a factor 8 (d + 8) / (5 d + 8) >= 1.6 resp. 4 (d + 8) / (3 d + 3) >= 1.33 to spare instead of
// about two.  That factor still pays for everything formed in fp32: qn2 and xn2 are off |q|^2, |x|^2 by at most d u relative, so
// fl(qn2 + xn2) >= S (1 - (d + 1) u) and fl(sqrt qn2) fl(sqrt xn2) >= P (1 - (d + 3) u); e itself takes three roundings, lo and hi one
// each of at most u (|a| + e) <= 2.1 u S: together below (d + 9) u of e's argument, against the 0.6 resp. 0.33 of it left over -- at
// d = 4096, 8 (d + 8) (1 - (d + 9) u) = 32824 > 5 d + 8 + 5 = 20493, and 4 (d + 8) (1 - (d + 9) u) = 16412 > 3 d + 3 + 3 = 12294; at
// d = 16, 191 > 93 and 95 > 54.  The constants are 4r's: nothing is lowered.
// Subnormal halves: whether the matrix pipeline reads them or flushes them to zero is not established, so the margin holds either
// way.  A flushed operand loses at most 2^-14 |other_i| of p at its position; with mq, mx the numbers of nonzero elements of magnitude
// below 2^-14 in q and x, Cauchy-Schwarz bounds the lost part of p by
//   lost = 2^-14 (sqrt(mx) |q| + sqrt(mq) |x|) + min(mq, mx) 2^-28
// (the last term a position where both are subnormal, counted once more than needed).  e grows by lost (IP) or 2 lost (L2), formed
// from the fp32 norms and scaled by 1 + 2^-10 against their d u and its own roundings.  mq == mx == 0 returns exact_screen_margin's
// value itself, bit for bit: ordinary data pays nothing, and the screen's pre-test (below) leans on that.
// No underflow beyond that: a nonzero product is at least 2^-48, a sum at most 2^44.  +inf as above.
HS_HD float exact_screen_f16_margin(int metric_ip, uint32_t dim, float qn2, float xn2, uint32_t mq, uint32_t mx) {
  const float e = exact_screen_margin(metric_ip, dim, qn2, xn2);
  if ((mq | mx) == 0u) return e;
  const float lost = 6.1035156e-5f * (__builtin_sqrtf((float)mx) * __builtin_sqrtf(qn2) + __builtin_sqrtf((float)mq) * __builtin_sqrtf(xn2)) +
                     (float)(mq < mx ? mq : mx) * 3.7252903e-9f;   // 2^-14, 2^-28
  return e + (metric_ip ? 1.0009766f : 2.0019531f) * lost;         // (1 + 2^-10), 2 (1 + 2^-10)
}

// The pre-test of exact_screen_f16q.hip: one FMA and one compare per accumulator element that may only OVER-admit -- what passes still
// meets the full test lo <= U, so a pair the pre-test drops must be one the full test drops.  It serves pairs with mq == mx == 0 and
// finite norms (everything else goes to the full test), where lo = fl(a - e) with e = exact_screen_margin.  With |p| <= 1.01 |q| |x|
// (the dot's own error bound) every rounding below is relative to at most 2.1 S resp. 1.01 (P' + 1), P' = fl(sqrt qn2) fl(sqrt xn2):
//   L2  lo >= (qn2 + xn2) - 2 p - [u + 4.3 u (1 + u)] (qn2 + xn2) - e (1 + u),  e (1 + u) <= 8 c (qn2 + xn2) (1 + u)^4 + 2 tiny
//          >= (qn2 + xn2) (1 - kL) - 2 p - 2 tiny,   kL = 8 (d + 9) u
//   IP  lo >= 1 - p - (P' + 1) kI - 3 tiny,          kI = 4 (d + 9) u
// In floats, with w = 1 - 8 (d + 10) u (exact) and up(t) = fl(t + 2^-20 |t|) >= t + 14 u |t| (it outweighs the rounding of t):
//   L2  row share  xlo = fl(fl(xn2 w) - 4 tiny) <= xn2 (1 - kL) - 2 tiny;  query share qlo = fl(qn2 w) <= qn2 (1 - kL);
//       bound      T = up(fl(U - qlo)) >= U - qlo;                          pre = fl(xlo - 2 p)       (one FMA)
//   IP  row share  sx = fl(sqrt xn2), the very value e is formed from;     query share g = -(up(fl(kI' sq)) + tiny), kI' = 4 (d + 10) u;
//       bound      T = up(fl(up(fl(U - 1)) + kI')) >= U - 1 + kI + 3 tiny;  pre = fl(g sx - p)        (one FMA)
// If lo <= U then, in real numbers, xlo - 2 p <= U - qlo <= T resp. g sx - p <= -kI P' - p <= U - 1 + kI + 3 tiny <= T; rounding is
// monotone and T is a float, so pre <= T as well.  Hence pre > T implies lo > U: the pair could not have entered the list.  The test is
// written !(pre > T) so that a NaN passes; U = +inf (a list below k rows) gives T = +inf by the same arithmetic.
HS_HD float exact_screen_f16_up(float t) { return __builtin_fmaf(__builtin_fabsf(t), 9.5367432e-7f, t); }
// the row's operand of the FMA: L2 xlo, IP sx
HS_HD float exact_screen_f16_pre_row(int metric_ip, uint32_t dim, float xn2) {
  if (metric_ip) return __builtin_sqrtf(xn2);
  const float w = 1.f - (float)(dim + 10u) * 4.7683716e-7f;   // 8 (d + 10) 2^-24, exact
  return xn2 * w - 4.f * ((float)(dim + 8u) * 7.5231638e-37f);
}
// the query's share: L2 qlo, IP g
HS_HD float exact_screen_f16_pre_query(int metric_ip, uint32_t dim, float qn2) {
  if (metric_ip) return -(exact_screen_f16_up((float)(dim + 10u) * 2.3841858e-7f * __builtin_sqrtf(qn2)) + (float)(dim + 8u) * 7.5231638e-37f);
  return qn2 * (1.f - (float)(dim + 10u) * 4.7683716e-7f);
}
// the bound a list with k-th hi U sets for the query (share: exact_screen_f16_pre_query)
HS_HD float exact_screen_f16_pre_bound(int metric_ip, uint32_t dim, float U, float share) {
  if (metric_ip) return exact_screen_f16_up(exact_screen_f16_up(U - 1.f) + (float)(dim + 10u) * 2.3841858e-7f);
  return exact_screen_f16_up(U - share);
}

// The bf16 screen of exact_screen_bf16q.hip: rows and queries are bf16 values -- fp32 values whose low 16 bits are zero
// -- the dot product p comes from v_mfma_f32_32x32x16_bf16, the norms from fp32 sums of the widened values, a is formed as above.  Its
// margin is exact_screen_margin itself; there is no function of its own, and the argument is this.
// Rounding.  A product of two bf16 values has 8 x 8 = 16 significand bits, so it is exact in fp32 wherever it does not underflow, and the
// fp16 screen's accounting holds word for word under the same premise (each addition of the pipeline errs by at most one ulp, in any
// order):  L2 |a - r| <= (5 d + 8) u S,  IP (3 d + 3) u (P + 1),  with the same factors to spare and the same (d + 9) u of them spent on
// S, P, e, lo and hi being formed in fp32.  No overflow where e is finite: S <= 2^125 resp. P <= 2^125 bound every product and, with the
// additions' error, every partial sum below 2^126.
// Underflow.  This is where bf16 is not fp16: the exponents are fp32's, so a product may fall below 2^-126, and a nonzero input may lie
// below 2^-126 (the bf16 subnormals k 2^-133) and be flushed to zero by the pipeline.  Whether any of that is flushed is not established,
// so every case is charged its worst absolute error, added to the relative bounds above:
//   a product below 2^-126, rounded to a subnormal or flushed          < 2^-126 per position, d 2^-126 in p
//   a sum of the pipeline that lands below 2^-126 and is flushed       < 2^-126 per addition (unflushed it is exact), d 2^-126 in p
//   an input below 2^-126 read as zero                                 its product, < 2^-126 |other_i|; over a vector, by
//                                                                      Cauchy-Schwarz, < 2^-126 sqrt(d) (|q| + |x|) in p
//   the squares of the two norms and the recipe's own terms            < 2^-126 each, 3 d 2^-126 together (already 4r's)
// With sqrt(d) <= 64 and t <= 1 + t^2, |q| + |x| <= 2 + S.  L2 doubles p:
//   extra(L2) <= 7 d 2^-126 + 2^-125 sqrt(d) (2 + S) <= (7 d + 4 sqrt(d)) 2^-126 + 2^-119 S <= 11 d 2^-126 + 2^-95 u S.
// The first part is below (d + 8) 2^-120 = 64 (d + 8) 2^-126, the `tiny` term of exact_screen_margin; the second is 2^-95 of one u S
// where more than 90 u S are spare (at d = 16; more above).  IP: e is finite only for finite norms, so |q|, |x| < 2^64 and
//   extra(IP) <= 4 d 2^-126 + 2^-126 sqrt(d) 2^65 <= (d + 8) 2^-120 + 2^-55,
// and 2^-55 is 2^-31 of one u (P + 1), P + 1 >= 1, where more than 40 u (P + 1) are spare.  So the expression of exact_screen_margin --
// (d + 8) 2^-120 included, nothing added -- bounds |a - r| for every (S, P) at which it is finite.  Overflow needs no term: S or P above
// 2^125 gives +inf above and the query falls back, as does a query that holds NaN or +-inf (its norm is not finite).
// The pre-test carries over, with one guard.  Its proof is about float arithmetic on the very p the full test uses -- lo <= U implies
// pre <= T whatever p's error -- and uses of the data only |p| <= 1.01 |q| |x|, so that the roundings of a stay relative to 2.1 S resp.
// 1.01 (P' + 1).  Here |p| <= 1.01 |q| |x| + extra.  IP: extra <= 2^-55 beside P' + 1 >= 1, far inside the 4 u (P' + 1) between kI' and
// kI.  L2: extra <= 2^-118 + 2^-119 S is small beside S only while S is not itself tiny, so a query with qn2 < 2^-40 skips the pre-test
// (every pair of it meets the full test); with S >= qn2 >= 2^-40, extra <= 2^-77 S, far inside the 7 u S between w and 1 - kL.  Products
// of the pre-test's own floats that underflow (xn2 w for a tiny row) err by at most 2^-149, inside the 2 tiny its row share gives away.
// Rows of huge norm.  The pre-test above is stated for finite norms, and a query whose norm is not finite takes the full test; a bf16
// ROW, though, may hold 2^64 and more, so xn2 may exceed 2^125 or be +inf while the row still takes the pre-test (nothing is counted per
// row).  The full test of such a pair has e = +inf, sets the fallback flag and admits nothing, so dropping the pair is right only if
// the flag is not needed -- that is, if the pair's true value r is above U, U finite.  L2: xlo = fl(xn2 w - 4 tiny) is +inf or at least
// 2^124, pre = fl(xlo - 2 p) is +inf, huge, or NaN (p = +-inf or NaN); NaN passes, and pre > T happens only for finite T, where the real
// inequality of the proof (lo <= U implies xlo - 2 p <= T, with the real-valued lo = r - e' for any e' the relative bounds give) still
// reads r > U: the row is farther than the k-th upper bound by the same argument as for finite norms, overflow of xn2 to +inf only
// raising xlo.  IP: g <= 0 and sx = +inf or huge give pre = -inf, NaN or a value below -kI P' - p, so !(pre > T) holds and the pair
// passes to the full test, which flags the query.  Either way no pair is dropped whose full test would have changed the answer.
HS_HD bool exact_screen_bf16_pre_skip(int metric_ip, float qn2) { return !metric_ip && qn2 < 9.0949470e-13f; }   // 2^-40

// The fp8 screen of exact_screen_f8q.hip: rows and queries are OCP E4M3 bytes, the dot product p comes from
// v_mfma_f32_32x32x64_f8f6f4 (both operands E4M3, unscaled), the norms from fp32 sums of the widened values, a is formed as above.
// Products.  An E4M3 value is +-m 2^e with a 4-bit significand m (subnormals: 3 bits), 2^-9 <= |v| <= 448.  A product of two has at
// most 8 significand bits and magnitude in [2^-18, 448^2 = 200704]: exact in fp32, never subnormal there, never near overflow.
// Only the accumulation rounds.  So the fp16 screen's accounting holds word for word under the same premise (each addition of the
// pipeline errs by at most one ulp, in any order):  L2 |a - r| <= (5 d + 8) u S,  IP (3 d + 3) u (P + 1), with the same factors to
// spare and the same (d + 9) u of them spent on S, P, e, lo and hi being formed in fp32.  Range: |q.x| <= d 448^2 < 2^30 and the norms
// are below 2^30 at d <= 4096, every partial sum with them; a nonzero partial sum is a multiple of 2^-18, so nothing underflows.  The
// recipe's own squares (t = q - x is a multiple of 2^-9, t^2 of 2^-18) and products do not underflow either, so exact_screen_margin's
// (d + 8) 2^-120 term is not drawn on at all.  Hence exact_screen_margin covers the screen as it stands whenever the pipeline reads
// every input byte as the value it encodes.
// Subnormal bytes.  Whether the matrix pipeline reads the E4M3 subnormals (+-k 2^-9, k = 1 .. 7, exponent field 0) or flushes them to
// zero could not be established without a measurement that this margin must not depend on, so -- as for the fp16 screen -- the
// margin holds either way and the counted term is added: a flushed operand loses at most 2^-6 |other_i| of p at its position, and
// with mq, mx the numbers of subnormal bytes in q and x Cauchy-Schwarz bounds the lost part of p by
//   lost = 2^-6 (sqrt(mx) |q| + sqrt(mq) |x|) + min(mq, mx) 2^-12.
// e grows by lost (IP) or 2 lost (L2), scaled by 1 + 2^-10 as in exact_screen_f16_margin.  mq == mx == 0 returns exact_screen_margin's
// value bit for bit, which is what the pre-test (above) is stated for: it serves the pairs without subnormal bytes and with finite
// norms, everything else takes the full test, and its proof uses of the data only |p| <= 1.01 |q| |x|, which the rounding bound gives.
// A query that holds a NaN byte has a NaN norm: e = +inf and the query falls back.  There are no infinities in the format.
HS_HD float exact_screen_f8_margin(int metric_ip, uint32_t dim, float qn2, float xn2, uint32_t mq, uint32_t mx) {
  const float e = exact_screen_margin(metric_ip, dim, qn2, xn2);
  if ((mq | mx) == 0u) return e;
  const float lost = 0.015625f * (__builtin_sqrtf((float)mx) * __builtin_sqrtf(qn2) + __builtin_sqrtf((float)mq) * __builtin_sqrtf(xn2)) +
                     (float)(mq < mx ? mq : mx) * 2.4414062e-4f;   // 2^-6, 2^-12
  return e + (metric_ip ? 1.0009766f : 2.0019531f) * lost;         // (1 + 2^-10), 2 (1 + 2^-10)
}

}  // namespace hs
