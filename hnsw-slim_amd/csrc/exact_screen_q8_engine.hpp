// exact_screen_q8_engine.hpp -- launch interface of the exact search for byte queries over byte rows (exact_screen_q8.hip):
// the screen of exact_screen.hip with the distance of every (query, row) pair computed exactly on the integer matrix cores, the same
// candidate lists, the same re-rank and fallback behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_screen_engine.hpp"

namespace hs {

// What the pack kernel leaves per query: qa the query's share of the screen's integer (L2: the norm of the bytes as the MFMA sees them;
// IP: minus the u8 shift terms, 0 for i8), qn the squared norm of the true values, floor_lo exact_screen_q8_inexact_floor.
struct XqQuery { int32_t qa; uint32_t qn; float floor_lo; uint32_t pad; };
// ... and the row-norm kernel per row: the squared norm and the sum of the bytes as the MFMA sees them (u8: the value minus 128)
struct XqRow { uint32_t norm; int32_t sum; };

// Workspace of a call, beside ScreenArgs' (whose xnorm2 / qnorm2 stay unused and whose x.queries must be `wide`).
struct XqArgs {
  const void *queries;   // x.nq x dim bytes in natural order, the format of the rows (device)
  uint8_t *packed;       // x.nq x dim: the queries in the narrow copy's slot order, u8 with the sign bit flipped
  float *wide;           // x.nq x dim: the queries as fp32, for the re-rank and the fallback scan
  XqQuery *qinfo;        // x.nq
  const XqRow *rinfo;    // ix.n, written by launch_exact_q8_rownorms once per call
};

// Byte rows (ROWS_U8 / ROWS_I8), dim % 32 == 0, dim <= 4096, 1 <= k <= 64; anything else is widened and handed to exact_screen.hip.
bool xq_supported(int fmt, uint32_t dim, uint32_t k);
// Positions of the query tile held in LDS at a time (dim, or slices of 256), and the kernel's dynamic LDS.
uint32_t xq_slice(uint32_t dim);
size_t xq_screen_lds_bytes(uint32_t dim, uint32_t k);
const char *xq_kernel_name(int fmt);
hipError_t launch_exact_q8_rownorms(const DevIndex &ix, const void *rows, int fmt, XqRow *rinfo, hipStream_t stream);
// count values of `src` (fmt bytes) as fp32: the hand-over to the fp32 screen
hipError_t launch_exact_q8_widen(const void *src, int fmt, size_t count, float *dst, hipStream_t stream);
// Pack, screen, re-rank, fallback of one group (geometry: xs_plan); all enqueued, nothing read back.
hipError_t launch_exact_screen_q8(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const XqArgs &q, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
