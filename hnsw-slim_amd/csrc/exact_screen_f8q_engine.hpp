// exact_screen_f8q_engine.hpp -- launch interface of the exact search for fp8 (OCP E4M3) queries over fp8 rows (exact_screen_f8q.hip,
// DESIGN.md 4w): the screen of exact_screen.hip with the dot products on the fp8 matrix cores (v_mfma_f32_32x32x64_f8f6f4), the same
// candidate lists, the same re-rank and fallback behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_screen_f16q_engine.hpp"

namespace hs {

// The five entries of exact_screen_f16q_engine.hpp for ROWS_F8, with that header's XhInfo and XhArgs: `queries` and `packed` are then
// E4M3 bytes (nq x dim of them; the uint16_t pointer is only a base address), XhInfo.sub counts the nonzero bytes of magnitude below
// 2^-6 (exact_screen_margin.hpp, exact_screen_f8_margin).  fp8 rows, dim % 16 == 0, dim <= 4096, 1 <= k <= 64; anything else is
// widened and handed to exact_screen.hip's route.
bool xf_supported(int fmt, uint32_t dim, uint32_t k);
// Positions of the query tile held in LDS at a time (dim, or slices of 256), and the kernel's dynamic LDS.
uint32_t xf_slice(uint32_t dim, uint32_t k);
size_t xf_screen_lds_bytes(uint32_t dim, uint32_t k);
const char *xf_kernel_name();
hipError_t launch_exact_f8q_rowinfo(const DevIndex &ix, const void *rows, XhInfo *rinfo, hipStream_t stream);
// count bytes of `src` as fp32: the hand-over to the fp32 queries' route
hipError_t launch_exact_f8q_widen(const void *src, size_t count, float *dst, hipStream_t stream);
// Pack, screen, re-rank, fallback of one group (geometry: xs_plan); all enqueued, nothing read back.
hipError_t launch_exact_screen_f8q(const DevIndex &ix, const void *rows, const ScreenArgs &a, const XhArgs &q, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
