// exact_screen_f16q_engine.hpp -- launch interface of the exact search for fp16 queries over fp16 rows (exact_screen_f16q.hip, DESIGN.md
// 4u): the screen of exact_screen.hip with the dot products on the half-precision matrix cores (v_mfma_f32_32x32x16_f16), the same
// candidate lists, the same re-rank and fallback behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_screen_engine.hpp"

namespace hs {

// What the pack kernel leaves per query and the row kernel per row: the fp32 squared norm, summed as xs_norms_kernel sums a narrow
// vector, and the number of nonzero elements of magnitude below 2^-14 (exact_screen_margin.hpp, exact_screen_f16_margin).
struct XhInfo { float norm; uint32_t sub; };

// Workspace of a call, beside ScreenArgs' (whose xnorm2 / qnorm2 stay unused and whose x.queries must be `wide`).
struct XhArgs {
  const void *queries;   // x.nq x dim halves in natural order (device)
  uint16_t *packed;      // x.nq x dim: the queries in the narrow copy's slot order
  float *wide;           // x.nq x dim: the queries as fp32, for the re-rank and the fallback scan
  XhInfo *qinfo;         // x.nq
  const XhInfo *rinfo;   // ix.n, written by launch_exact_f16q_rowinfo once per call
};

// fp16 rows (ROWS_F16), dim % 16 == 0, dim <= 4096, 1 <= k <= 64; anything else is widened and handed to exact_screen.hip's route.
bool xh_supported(int fmt, uint32_t dim, uint32_t k);
// Positions of the query tile held in LDS at a time (dim, or slices of 256), and the kernel's dynamic LDS.
uint32_t xh_slice(uint32_t dim, uint32_t k);
size_t xh_screen_lds_bytes(uint32_t dim, uint32_t k);
const char *xh_kernel_name();
hipError_t launch_exact_f16q_rowinfo(const DevIndex &ix, const void *rows, XhInfo *rinfo, hipStream_t stream);
// count halves of `src` as fp32: the hand-over to the fp32 queries' route
hipError_t launch_exact_f16q_widen(const void *src, size_t count, float *dst, hipStream_t stream);
// Pack, screen, re-rank, fallback of one group (geometry: xs_plan); all enqueued, nothing read back.
hipError_t launch_exact_screen_f16q(const DevIndex &ix, const void *rows, const ScreenArgs &a, const XhArgs &q, const FilterArgs *f, hipStream_t stream);

// The same five for bf16 queries over bf16 rows (ROWS_BF16; exact_screen_bf16q.hip, DESIGN.md 4v: v_mfma_f32_32x32x16_bf16).  XhArgs
// and XhInfo serve both: `queries` and `packed` are then bf16 words, and XhInfo.sub is zero (the bf16 margin counts nothing).
bool xb_supported(int fmt, uint32_t dim, uint32_t k);
uint32_t xb_slice(uint32_t dim, uint32_t k);
size_t xb_screen_lds_bytes(uint32_t dim, uint32_t k);
const char *xb_kernel_name();
hipError_t launch_exact_bf16q_rowinfo(const DevIndex &ix, const void *rows, XhInfo *rinfo, hipStream_t stream);
hipError_t launch_exact_bf16q_widen(const void *src, size_t count, float *dst, hipStream_t stream);
hipError_t launch_exact_screen_bf16q(const DevIndex &ix, const void *rows, const ScreenArgs &a, const XhArgs &q, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
