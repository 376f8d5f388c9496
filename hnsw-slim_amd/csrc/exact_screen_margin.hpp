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

}  // namespace hs
