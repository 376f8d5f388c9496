// search_launch.cpp -- launch_search (engine.hpp): the one way from a launch plan to a search kernel.  Host only: the table of the
// kernel objects' launchers by family, row format and metric, and the refusals that hold for every cell of it.
#include "../../include/hnsw_slim_amd.h"
#include "dist_recipe.hpp"
#include "engine.hpp"
#include "narrow_rows.hpp"

namespace hs {

// [hs_plan_family][ROWS_*][metric].  (The row formats in ROWS_* order -- f32, f16, u8 -- which is not the kernel files' HS_TU_ROWS.)
static constexpr SearchLauncher kLaunchers[4][3][2] = {
    /* HS_PLAN_FLAT   */ {{HS_LAUNCHERS(flat, f32)}, {HS_LAUNCHERS(flat, f16)}, {HS_LAUNCHERS(flat, u8)}},
    /* HS_PLAN_LEAN   */ {{HS_LAUNCHERS(lean, f32)}, {}, {}},   // (no narrow twin)
    /* HS_PLAN_FAST   */ {{HS_LAUNCHERS(fast, f32)}, {HS_LAUNCHERS(fast, f16)}, {HS_LAUNCHERS(fast, u8)}},
    /* HS_PLAN_STRICT */ {{HS_LAUNCHERS(strict, f32)}, {HS_LAUNCHERS(strict, f16)}, {HS_LAUNCHERS(strict, u8)}},
};
static_assert(HS_PLAN_FLAT == 0 && HS_PLAN_LEAN == 1 && HS_PLAN_FAST == 2 && HS_PLAN_STRICT == 3, "the table's rows are in hs_plan_family order");
static_assert(ROWS_F32 == 0 && ROWS_F16 == 1 && ROWS_U8 == 2 && METRIC_L2 == 0 && METRIC_IP == 1, "the table's columns are in ROWS_* / Metric order");
// every cell but the lean kernel's four narrow ones holds a launcher (one that no object defines does not link)
static constexpr bool table_complete() {
  for (int fam = 0; fam < 4; fam++)
    for (int fmt = 0; fmt < 3; fmt++)
      for (int m = 0; m < 2; m++)
        if ((kLaunchers[fam][fmt][m] == nullptr) != (fam == HS_PLAN_LEAN && fmt != ROWS_F32)) return false;
  return true;
}
static_assert(table_complete(), "a search launcher is missing from the table");

hipError_t launch_search(int family, int row_fmt, const DevIndex &ix, const SearchArgs &a, const void *narrow_rows, hipStream_t stream,
                         const FilterArgs *f) {
  if (family < 0 || family > 3 || row_fmt < 0 || row_fmt > 2 || ix.metric < 0 || ix.metric > 1) return hipErrorInvalidValue;
  const SearchLauncher go = kLaunchers[family][row_fmt][ix.metric];
  if (go == nullptr) return hipErrorInvalidValue;
  if (f != nullptr && (family == HS_PLAN_FLAT || family == HS_PLAN_LEAN)) return hipErrorInvalidValue;   // no filter-set form; the plan never asks
  const void *rows = row_fmt == ROWS_F32 ? ix.vec : narrow_rows;
  // (an index may have dropped its fp32 rows, hs_index_set_f32_resident, or never made a narrow copy: refused here instead of
  //  dereferencing null on the device)
  if (rows == nullptr && ix.n > 0) return hipErrorInvalidDevicePointer;
  if (row_fmt != ROWS_F32 && (ix.dim & 15u) != 0) return hipErrorInvalidValue;   // the lane-major layout needs whole 16-element steps
  return go(ix, a, narrow_rows, stream, f);
}

}  // namespace hs
