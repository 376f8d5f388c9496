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

}  // namespace hs
